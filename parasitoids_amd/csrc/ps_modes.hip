// Ensemble modes (include/parasitoid_hip.h, ps_modes_*): the members' transformed fields kept on the device, their
// weighted mean plane, the M x M table of inner products of the (centred) fields and linear combinations of them.
// The value of a slot is the one ps_summary_add adds (ps_record_value); X = v or sqrt(v).  Layout (pitch = N*N
// rounded up to 64 cells, as ps_summary.hip):
//   X[member][slot][pitch]     fp64, the pad cells 0; grows by doubling
//   mu[slot][pitch]            fp64, the weighted mean, cached per slot until the next add, merge or reset
//   part[split][M][M]          fp64, the partial tables of the splits of the cell axis
//   tab[M][M]                  fp64, their sum in split order
//   win[2]                     uint32, the live window [first, last + 1) of the plane in words of 64 cells
// k_modes_gram is a symmetric fp64 product on the matrix units (v_mfma_f64_16x16x4_f64): a workgroup owns one pair
// of member tiles (ti <= tj) and every gridDim.y-th chunk of the cell range, stages both tiles' cells of a chunk
// through LDS -- the mean subtracted on the way in -- and each of its four waves keeps a 32 x 32 block of the table
// in four accumulators.  No floating-point atomics: every split writes its own partial table and k_modes_reduce
// adds them in split order, so two calls return the same bits.  No inline assembly.
#include <math.h>

#include <algorithm>
#include <vector>

#include "ps_common.h"

#define PS_MOD_MAX_SLOT 8
#define PS_MOD_MAX_COEF 8
#define PS_MOD_THREADS 256
#define PS_MOD_MEMBERS0 4                 // members allocated by the first add that finds no room
#define PS_MOD_TILE 64                    // members per tile edge: 2 x 2 waves of 32 x 32, each 2 x 2 MFMA tiles
#define PS_MOD_KC 32                      // cells of one staged chunk
#define PS_MOD_ROW (PS_MOD_KC + 2)        // LDS row in doubles: 16 rows x 2 cells of one half-wave fall on 32 distinct double banks
#define PS_MOD_STAGE (PS_MOD_TILE * PS_MOD_KC / PS_MOD_THREADS)   // doubles of each tile a thread stages per chunk
#define PS_MOD_BLOCKS 1024                // the workgroups a launch stays within: 4 per CU

namespace {

typedef double modes_d4 __attribute__((ext_vector_type(4)));

struct ModSlots {
  PsSrc s[PS_MOD_MAX_SLOT];
};

// thread i owns cell i of every slot; the grid covers the pitch, so the pad cells get their zeros
__global__ void __launch_bounds__(PS_MOD_THREADS) k_modes_add(ModSlots desc, int nslot, double* __restrict__ X,
                                                              int64_t ncell, int64_t pitch, double negval, int root) {
  __shared__ double sdelta[PS_MOD_MAX_SLOT];
  for (int t = threadIdx.x; t < nslot; t += blockDim.x) sdelta[t] = desc.s[t].stats ? desc.s[t].stats->delta : 0.0;
  __syncthreads();
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= pitch) return;
  const bool real = i < ncell;
  for (int s = 0; s < nslot; ++s) {
    const PsSrc& sd = desc.s[s];
    double v = 0.0;
    if (real) v = ps_record_value(sd.rec[i], sd.stat_scale, sd.post_scale, sdelta[s], negval);
    X[(int64_t)s * pitch + i] = root ? __dsqrt_rn(v) : v;
  }
}

// thread i owns cell i: acc += w_m X_m in add order, multiply and add rounded separately, one division at the end
__global__ void __launch_bounds__(PS_MOD_THREADS) k_modes_mean(const double* __restrict__ X, int64_t member_stride,
                                                               int64_t members, const double* __restrict__ w, double W,
                                                               int64_t pitch, double* __restrict__ mu) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= pitch) return;
  double acc = 0.0;
  for (int64_t m = 0; m < members; ++m) acc = __dadd_rn(acc, __dmul_rn(w[m], X[m * member_stride + i]));
  mu[i] = acc / W;
}

// the first and one past the last word of 64 cells in which the mean is non-zero: outside them every member is zero
// (X >= 0 and w >= 1, so a sum that is zero has zero terms only).  win = {0xffffffff, 0} before.
__global__ void __launch_bounds__(PS_MOD_THREADS) k_modes_window(const double* __restrict__ mu, int64_t pitch,
                                                                 uint32_t* __restrict__ win) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;   // a multiple of 64, as the pitch: whole waves
  uint32_t lo = 0xffffffffu, hi = 0u;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < pitch; i += stride) {
    if (__any(mu[i] != 0.0)) {
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

// blockIdx.x: the tile pair (ti <= tj) in row-major order of the upper triangle; blockIdx.y: the split.  Staging:
// thread (lr, lw) = (tid / 32, tid % 32) loads cell lw of the chunk for the members lr + 8 q of both tiles; members
// past M and cells past the range are stored as zeros.  Product: wave (wy, wx) owns the members 32 wy.. of tile ti
// against 32 wx.. of tile tj.  The f64 16x16x4 fragment: A and B one f64 per lane, member lane & 15, cell lane >> 4;
// C/D four f64 per lane, column lane & 15, row (lane >> 4) + 4 reg.  A diagonal tile writes the entries on and above
// the diagonal and their mirror images, any other tile its entry and the mirrored one: every entry of the split's
// partial table has one writer.
__global__ void __launch_bounds__(PS_MOD_THREADS) k_modes_gram(const double* __restrict__ X, int64_t member_stride,
                                                               const double* __restrict__ mu, int64_t M, int ntile,
                                                               const uint32_t* __restrict__ win, int64_t whole,
                                                               int64_t pitch, double* __restrict__ part) {
  __shared__ double sa[PS_MOD_TILE * PS_MOD_ROW];
  __shared__ double sb[PS_MOD_TILE * PS_MOD_ROW];
  int t = blockIdx.x, ti = 0;
  while (t >= ntile - ti) {
    t -= ntile - ti;
    ++ti;
  }
  const int tj = ti + t;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lw = tid & (PS_MOD_KC - 1), lr = tid / PS_MOD_KC;
  const int wy = (wave >> 1) * 32, wx = (wave & 1) * 32;
  const int fr = lane & 15, fk = lane >> 4;
  int64_t w0 = whole > 0 ? 0 : (int64_t)win[0], w1 = whole > 0 ? whole : (int64_t)win[1];   // whole: no window
  w1 = min(w1, pitch >> 6);
  const int64_t c0 = w0 * 64, c1 = w1 * 64;   // an empty window has w0 > w1: no chunk
  modes_d4 acc[2][2];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 2; ++c) acc[r][c] = modes_d4{0.0, 0.0, 0.0, 0.0};
  // every load is made, from an address clamped into the block, and zeroed afterwards where it is past the members
  // or the range.  The loads of the next chunk are issued once this one's values are in LDS and are waited for only
  // at the next store, so they fly while the matrix units work.
  const int64_t step = (int64_t)gridDim.y * PS_MOD_KC;
  int64_t base = c0 + (int64_t)blockIdx.y * PS_MOD_KC;
  int64_t cell = 0;
  double mean = 0.0;
  double va[PS_MOD_STAGE], vb[PS_MOD_STAGE];
  auto fetch = [&](int64_t b) {
    cell = b + lw;
    const int64_t cc = min(cell, c1 - 1);
    mean = mu ? mu[cc] : 0.0;
#pragma unroll
    for (int q = 0; q < PS_MOD_STAGE; ++q) {
      const int row = lr + q * (PS_MOD_THREADS / PS_MOD_KC);
      const int64_t ma = (int64_t)ti * PS_MOD_TILE + row, mb = (int64_t)tj * PS_MOD_TILE + row;
      va[q] = X[min(ma, M - 1) * member_stride + cc];
      vb[q] = X[min(mb, M - 1) * member_stride + cc];
    }
  };
  if (base < c1) fetch(base);
  for (; base < c1; base += step) {
#pragma unroll
    for (int q = 0; q < PS_MOD_STAGE; ++q) {
      const int row = lr + q * (PS_MOD_THREADS / PS_MOD_KC);
      const int64_t ma = (int64_t)ti * PS_MOD_TILE + row, mb = (int64_t)tj * PS_MOD_TILE + row;
      const double xa = mu ? va[q] - mean : va[q], xb = mu ? vb[q] - mean : vb[q];
      sa[row * PS_MOD_ROW + lw] = (ma < M && cell < c1) ? xa : 0.0;
      sb[row * PS_MOD_ROW + lw] = (mb < M && cell < c1) ? xb : 0.0;
    }
    __syncthreads();
    if (base + step < c1) fetch(base + step);
#pragma unroll
    for (int k = 0; k < PS_MOD_KC; k += 4) {
      double a[2], b[2];
#pragma unroll
      for (int r = 0; r < 2; ++r) a[r] = sa[(wy + 16 * r + fr) * PS_MOD_ROW + k + fk];
#pragma unroll
      for (int c = 0; c < 2; ++c) b[c] = sb[(wx + 16 * c + fr) * PS_MOD_ROW + k + fk];
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[r][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[r], b[c], acc[r][c], 0, 0, 0);
    }
    __syncthreads();   // the next chunk overwrites the tiles
  }
  double* out = part + (int64_t)blockIdx.y * M * M;
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int64_t i = (int64_t)ti * PS_MOD_TILE + wy + 16 * r + fk + 4 * g;
        const int64_t j = (int64_t)tj * PS_MOD_TILE + wx + 16 * c + fr;
        if (i < M && j < M && (ti != tj || i <= j)) {
          out[i * M + j] = acc[r][c][g];
          if (i != j) out[j * M + i] = acc[r][c][g];
        }
      }
}

// one thread per entry: the partial tables added in split order
__global__ void __launch_bounds__(PS_MOD_THREADS) k_modes_reduce(const double* __restrict__ part, int64_t n, int split,
                                                                 double* __restrict__ tab) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  double acc = part[i];
  for (int s = 1; s < split; ++s) acc += part[(int64_t)s * n + i];
  tab[i] = acc;
}

// thread i owns cell i of every output: out_k += coef_km A_m in add order, multiply and add rounded separately; a
// member is read once for all outputs
__global__ void __launch_bounds__(PS_MOD_THREADS) k_modes_combine(const double* __restrict__ X, int64_t member_stride,
                                                                  const double* __restrict__ mu, int64_t members,
                                                                  const double* __restrict__ coef, int ncoef,
                                                                  int64_t pitch, double* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= pitch) return;
  const double mean = mu ? mu[i] : 0.0;
  double acc[PS_MOD_MAX_COEF];
#pragma unroll
  for (int k = 0; k < PS_MOD_MAX_COEF; ++k) acc[k] = 0.0;
  for (int64_t m = 0; m < members; ++m) {
    const double x = X[m * member_stride + i];
    const double a = mu ? x - mean : x;
#pragma unroll
    for (int k = 0; k < PS_MOD_MAX_COEF; ++k)
      if (k < ncoef) acc[k] = __dadd_rn(acc[k], __dmul_rn(coef[(int64_t)k * members + m], a));
  }
#pragma unroll
  for (int k = 0; k < PS_MOD_MAX_COEF; ++k)
    if (k < ncoef) out[(int64_t)k * pitch + i] = acc[k];
}

}  // namespace

struct ps_modes {
  int device = 0, N = 0, nslot = 0, transform = 0;
  int64_t ncell = 0, pitch = 0;
  double* X = nullptr;          // [cap][slot][pitch]
  int64_t cap = 0;
  double* mu = nullptr;         // [slot][pitch]
  bool mu_valid[PS_MOD_MAX_SLOT] = {false, false, false, false, false, false, false, false};
  double* wdev = nullptr;       // [wdev_cap] the weights as fp64, then the coefficients of one combine
  int64_t wdev_cap = 0;
  bool wdev_valid = false;
  double* part = nullptr;       // [part_cap] the partial tables, then the table
  int64_t part_cap = 0;
  double* maps = nullptr;       // [PS_MOD_MAX_COEF][pitch], allocated by the first combine
  uint32_t* win = nullptr;      // [2]
  bool use_window = true;
  uint64_t W = 0;
  int64_t members = 0;
  std::vector<uint32_t> weights;
  std::vector<double> host;     // staging of add_host and of the weights and coefficients
  hipStream_t stream = nullptr;
  PsLastOp last;
  PsProf prof;                  // channel 0: the adds, 1: the means, 2: the tables, 3: the combines
};

static int64_t mod_member_doubles(const ps_modes* a) { return (int64_t)a->nslot * a->pitch; }

static void mod_changed(ps_modes* a) {
  for (bool& v : a->mu_valid) v = false;
  a->wdev_valid = false;
}

// a device block of `bytes`, checked against the free memory first (who / what: for the message)
static int mod_alloc(void** p, double bytes, const char* who, const char* what) {
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (bytes > (double)free_b)
    return ps_fail(PS_ERR_OOM, "%s: %s need %.3g GB, %.3g GB free", who, what, bytes * 1e-9, (double)free_b * 1e-9);
  PS_HIP(hipMalloc(p, (size_t)bytes));
  return PS_OK;
}

// room for `need` members: exactly `need` when exact (ps_modes_reserve), else by doubling.  A growth copies the
// members so far on the handle's stream and synchronises once before the old block is freed.
static int mod_reserve_members(ps_modes* a, int64_t need, bool exact, const char* who) {
  if (need <= a->cap) return PS_OK;
  int64_t cap = need;
  if (!exact) {
    cap = std::max<int64_t>(a->cap, PS_MOD_MEMBERS0);
    while (cap < need) cap *= 2;
  }
  const double mem_b = (double)mod_member_doubles(a) * sizeof(double);
  double* p = nullptr;
  PS_TRY(mod_alloc((void**)&p, (double)cap * mem_b, who, "the members' fields"));
  if (a->X) {
    hipError_t e = hipSuccess;
    if (a->last.live) e = hipStreamWaitEvent(a->stream, a->last.ev, 0);
    if (e == hipSuccess && a->members > 0)
      e = hipMemcpyAsync(p, a->X, (size_t)((double)a->members * mem_b), hipMemcpyDeviceToDevice, a->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(a->stream);
    if (e != hipSuccess) {
      (void)hipFree(p);
      return ps_fail(PS_ERR_HIP, "%s: growing the members' fields: %s", who, hipGetErrorString(e));
    }
    PS_HIP(hipFree(a->X));
  }
  a->X = p;
  a->cap = cap;
  return PS_OK;
}

// a scratch block of at least `need` doubles, regrown (not copied) once the stream has drained
static int mod_scratch(ps_modes* a, double** p, int64_t* cap, int64_t need, const char* what) {
  if (need <= *cap) return PS_OK;
  if (*p) {
    PS_HIP(hipStreamSynchronize(a->stream));
    PS_HIP(hipFree(*p));
    *p = nullptr;
    *cap = 0;
  }
  PS_TRY(mod_alloc((void**)p, (double)need * sizeof(double), "modes", what));
  *cap = need;
  return PS_OK;
}

extern "C" void ps_modes_destroy(ps_modes* a) {
  if (!a) return;
  (void)hipSetDevice(a->device);
  a->last.sync();
  if (a->stream) (void)hipStreamSynchronize(a->stream);
  a->prof.release();
  for (void* p : {(void*)a->X, (void*)a->mu, (void*)a->wdev, (void*)a->part, (void*)a->maps, (void*)a->win})
    if (p) (void)hipFree(p);
  a->last.destroy();
  if (a->stream) (void)hipStreamDestroy(a->stream);
  delete a;
}

extern "C" int ps_modes_reset(ps_modes* a) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "modes_reset: null handle");
  a->W = 0;
  a->members = 0;
  a->weights.clear();
  mod_changed(a);
  return PS_OK;
}

extern "C" int ps_modes_create(int device, int N, int nslot, int transform, ps_modes** out) {
  if (!out || N < 1 || nslot < 1 || nslot > PS_MOD_MAX_SLOT)
    return ps_fail(PS_ERR_BAD_ARG, "modes_create: N %d, %d slots (1..%d)", N, nslot, PS_MOD_MAX_SLOT);
  *out = nullptr;
  if (transform != PS_MODES_RAW && transform != PS_MODES_SQRT)
    return ps_fail(PS_ERR_BAD_ARG, "modes_create: transform %d is neither raw (0) nor sqrt (1)", transform);
  PS_TRY(ps_use_device(device));
  const int64_t ncell = (int64_t)N * N;
  const int64_t pitch = (ncell + 63) / 64 * 64;
  if (pitch / PS_MOD_THREADS + 1 > 0x7fffffffLL)
    return ps_fail(PS_ERR_BAD_ARG, "modes_create: N %d is too large for one launch", N);
  // the mean planes, checked before anything is allocated; the members' fields are checked as they grow
  const double need = (double)nslot * pitch * 8.0;
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > (double)free_b)
    return ps_fail(PS_ERR_OOM, "modes_create: %d slots x %lld cells x 8 B = %.3g GB, %.3g GB free", nslot,
                   (long long)pitch, need * 1e-9, (double)free_b * 1e-9);
  ps_modes* a = new ps_modes();
  a->device = device;
  a->N = N;
  a->nslot = nslot;
  a->transform = transform;
  a->ncell = ncell;
  a->pitch = pitch;
  hipError_t e = hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = a->last.create();
  if (e == hipSuccess) e = hipMalloc((void**)&a->mu, (size_t)nslot * pitch * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&a->win, 2 * sizeof(uint32_t));
  if (e != hipSuccess) {
    ps_modes_destroy(a);
    return ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "modes_create: %s", hipGetErrorString(e));
  }
  *out = a;
  return PS_OK;
}

extern "C" int ps_modes_reserve(ps_modes* a, int64_t members) {
  if (!a || members < 0) return ps_fail(PS_ERR_BAD_ARG, "modes_reserve: bad arguments");
  PS_HIP(hipSetDevice(a->device));
  return mod_reserve_members(a, members, true, "modes_reserve");
}

extern "C" int ps_modes_set_window(ps_modes* a, int on) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "modes_set_window: null handle");
  a->use_window = on != 0;
  return PS_OK;
}

static int mod_check_weight(const ps_modes* a, const char* who, uint64_t weight) {
  if (weight < 1) return ps_fail(PS_ERR_BAD_ARG, "%s: weight must be >= 1", who);
  if (a->W + weight > 0xfffffffeull)
    return ps_fail(PS_ERR_BAD_ARG, "%s: total weight %llu would overflow: it has to stay below 2^32 - 1", who,
                   (unsigned long long)(a->W + weight));
  return PS_OK;
}

static void mod_added(ps_modes* a, uint32_t weight) {
  a->W += weight;
  a->members += 1;
  a->weights.push_back(weight);
  mod_changed(a);
}

// one member from the slot descriptors, enqueued on `stream`
static int mod_launch(ps_modes* a, const ModSlots& desc, hipStream_t stream, double negval, uint32_t weight,
                      const char* who) {
  PS_TRY(mod_reserve_members(a, a->members + 1, false, who));
  PS_TRY(a->last.wait(stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(0, stream, &e1));
  const unsigned nblk = (unsigned)((a->pitch + PS_MOD_THREADS - 1) / PS_MOD_THREADS);
  hipLaunchKernelGGL(k_modes_add, dim3(nblk), dim3(PS_MOD_THREADS), 0, stream, desc, a->nslot,
                     a->X + a->members * mod_member_doubles(a), a->ncell, a->pitch, negval,
                     a->transform == PS_MODES_SQRT ? 1 : 0);
  PS_HIP(hipGetLastError());
  PS_TRY(a->prof.end(stream, e1));
  PS_TRY(a->last.mark(stream));
  mod_added(a, weight);
  return PS_OK;
}

extern "C" int ps_modes_add(ps_modes* a, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                            const double* stat_scale, const double* post_scale, const int32_t* use_delta,
                            double negval, uint32_t weight) {
  if (!a || !s || !kind || !idx || !stat_scale || !post_scale || !use_delta)
    return ps_fail(PS_ERR_BAD_ARG, "modes_add: bad arguments");
  if (nslot != a->nslot)
    return ps_fail(PS_ERR_BAD_ARG, "modes_add: %d slots given, the handle has %d", nslot, a->nslot);
  PS_TRY(mod_check_weight(a, "modes_add", weight));
  PS_HIP(hipSetDevice(a->device));
  // every descriptor first: an add with a bad slot enqueues nothing
  ModSlots desc;
  hipStream_t stream = nullptr;
  PS_TRY(ps_read_records("modes_add", "handle", a->device, a->N, s, nslot, kind, idx, stat_scale, post_scale, use_delta,
                         false, desc.s, &stream));
  for (int i = nslot; i < PS_MOD_MAX_SLOT; ++i) desc.s[i] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  return mod_launch(a, desc, stream, negval, weight, "modes_add");
}

// one member whose slots are the current fields of a projection or a release plan, in ascending output order
static int mod_add_fields(ps_modes* a, void* h, const PsFieldsOps& src, const char* who, uint32_t weight) {
  if (!a || !h) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  PS_TRY(mod_check_weight(a, who, weight));
  // slot e takes Y_e: no statistics, both scales 1 and negval 0, so the value rule returns Y itself
  ModSlots desc;
  PS_TRY(ps_read_fields(who, "handle", "slots", a->device, a->N, a->nslot, h, src, desc.s));
  for (int e = a->nslot; e < PS_MOD_MAX_SLOT; ++e) desc.s[e] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(src.wait(h, a->stream));
  PS_TRY(mod_launch(a, desc, a->stream, 0.0, weight, who));
  return src.mark(h, a->stream);   // the next apply overwrites the source's fields only after this read
}

extern "C" int ps_modes_add_project(ps_modes* a, ps_project* p, uint32_t weight) {
  return mod_add_fields(a, p, ps_project_fields(), "modes_add_project", weight);
}

extern "C" int ps_modes_add_sites(ps_modes* a, ps_sites* p, uint32_t weight) {
  return mod_add_fields(a, p, ps_sites_fields(), "modes_add_sites", weight);
}

extern "C" int ps_modes_add_host(ps_modes* a, const double* fields, uint32_t weight) {
  if (!a || !fields) return ps_fail(PS_ERR_BAD_ARG, "modes_add_host: bad arguments");
  PS_TRY(mod_check_weight(a, "modes_add_host", weight));
  // every value first: a bad field stores nothing
  const int64_t n = (int64_t)a->nslot * a->ncell;
  for (int64_t i = 0; i < n; ++i)
    if (!(fields[i] >= 0.0) || !isfinite(fields[i]))
      return ps_fail(PS_ERR_BAD_ARG, "modes_add_host: value %g at slot %lld, cell %lld is negative or not finite",
                     fields[i], (long long)(i / a->ncell), (long long)(i % a->ncell));
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(mod_reserve_members(a, a->members + 1, false, "modes_add_host"));
  a->host.assign((size_t)mod_member_doubles(a), 0.0);
  for (int s = 0; s < a->nslot; ++s)
    for (int64_t i = 0; i < a->ncell; ++i) {
      const double v = fields[(int64_t)s * a->ncell + i];
      a->host[(size_t)(s * a->pitch + i)] = a->transform == PS_MODES_SQRT ? sqrt(v) : v;
    }
  PS_TRY(a->last.wait(a->stream));
  PS_HIP(hipMemcpyAsync(a->X + a->members * mod_member_doubles(a), a->host.data(), a->host.size() * sizeof(double),
                        hipMemcpyHostToDevice, a->stream));
  PS_TRY(a->last.mark(a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));   // the staging block is read until here
  mod_added(a, weight);
  return PS_OK;
}

extern "C" int ps_modes_merge(ps_modes* dst, ps_modes* src) {
  if (!dst || !src || dst == src) return ps_fail(PS_ERR_BAD_ARG, "modes_merge: bad arguments");
  if (dst->device != src->device || dst->N != src->N || dst->nslot != src->nslot || dst->transform != src->transform)
    return ps_fail(PS_ERR_BAD_ARG, "modes_merge: handles differ in device, domain, slots or transform");
  if (dst->W + src->W > 0xfffffffeull) return ps_fail(PS_ERR_BAD_ARG, "modes_merge: total weight would overflow");
  if (src->members == 0) return PS_OK;
  PS_HIP(hipSetDevice(dst->device));
  PS_TRY(mod_reserve_members(dst, dst->members + src->members, false, "modes_merge"));
  PS_TRY(dst->last.wait(dst->stream));
  PS_TRY(src->last.wait(dst->stream));
  const int64_t md = mod_member_doubles(dst);
  PS_HIP(hipMemcpyAsync(dst->X + dst->members * md, src->X, (size_t)(src->members * md) * sizeof(double),
                        hipMemcpyDeviceToDevice, dst->stream));
  PS_TRY(dst->last.mark(dst->stream));
  PS_TRY(src->last.mark(dst->stream));   // src is read until then
  dst->W += src->W;
  dst->members += src->members;
  dst->weights.insert(dst->weights.end(), src->weights.begin(), src->weights.end());
  mod_changed(dst);
  return PS_OK;
}

extern "C" int ps_modes_info(ps_modes* a, double* total_weight, int64_t* members, int64_t* capacity, int64_t* bytes) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "modes_info: null handle");
  if (total_weight) *total_weight = (double)a->W;
  if (members) *members = a->members;
  if (capacity) *capacity = a->cap;
  if (bytes)
    *bytes = (a->cap * mod_member_doubles(a) + mod_member_doubles(a) + a->wdev_cap + a->part_cap +
              (a->maps ? PS_MOD_MAX_COEF * a->pitch : 0) + 1) * (int64_t)sizeof(double);
  return PS_OK;
}

extern "C" int ps_modes_weights(ps_modes* a, int64_t members_expected, uint32_t* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "modes_weights: bad arguments");
  if (members_expected != a->members)
    return ps_fail(PS_ERR_BAD_ARG, "modes_weights: %lld members expected, the handle holds %lld",
                   (long long)members_expected, (long long)a->members);
  std::copy(a->weights.begin(), a->weights.end(), out);
  return PS_OK;
}

static int mod_check_slot(ps_modes* a, int slot, const char* who) {
  if (slot < 0 || slot >= a->nslot) return ps_fail(PS_ERR_BAD_ARG, "%s: slot %d of %d", who, slot, a->nslot);
  if (a->members == 0) return ps_fail(PS_ERR_STATE, "%s: nothing accumulated (no member added)", who);
  return PS_OK;
}

// the weights as fp64 at wdev[0..members), and room for `extra` doubles behind them; the caller has ordered the
// stream and synchronises before it returns (the staging block is read until then)
static int mod_weights_dev(ps_modes* a, int64_t extra) {
  const int64_t need = a->members + extra;
  if (need > a->wdev_cap) {
    int64_t cap = std::max<int64_t>(a->wdev_cap, 1024);
    while (cap < need) cap *= 2;
    PS_TRY(mod_scratch(a, &a->wdev, &a->wdev_cap, cap, "the weights"));
    a->wdev_valid = false;
  }
  if (!a->wdev_valid) {
    a->host.resize((size_t)a->members);
    for (int64_t m = 0; m < a->members; ++m) a->host[(size_t)m] = (double)a->weights[(size_t)m];
    PS_HIP(hipMemcpyAsync(a->wdev, a->host.data(), (size_t)a->members * sizeof(double), hipMemcpyHostToDevice, a->stream));
    PS_HIP(hipStreamSynchronize(a->stream));
    a->wdev_valid = true;
  }
  return PS_OK;
}

// the mean plane of `slot` on the device, current; the stream is ordered behind the last operation
static int mod_mean_dev(ps_modes* a, int slot) {
  PS_TRY(a->last.wait(a->stream));
  if (a->mu_valid[slot]) return PS_OK;
  PS_TRY(mod_weights_dev(a, 0));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(1, a->stream, &e1));
  const unsigned nblk = (unsigned)((a->pitch + PS_MOD_THREADS - 1) / PS_MOD_THREADS);
  hipLaunchKernelGGL(k_modes_mean, dim3(nblk), dim3(PS_MOD_THREADS), 0, a->stream, a->X + (int64_t)slot * a->pitch,
                     mod_member_doubles(a), a->members, a->wdev, (double)a->W, a->pitch, a->mu + (int64_t)slot * a->pitch);
  PS_HIP(hipGetLastError());
  PS_TRY(a->prof.end(a->stream, e1));
  PS_TRY(a->last.mark(a->stream));
  a->mu_valid[slot] = true;
  return PS_OK;
}

extern "C" int ps_modes_mean(ps_modes* a, int slot, double* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "modes_mean: bad arguments");
  PS_TRY(mod_check_slot(a, slot, "modes_mean"));
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(mod_mean_dev(a, slot));
  PS_HIP(hipMemcpyAsync(out, a->mu + (int64_t)slot * a->pitch, (size_t)a->ncell * sizeof(double), hipMemcpyDeviceToHost,
                        a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  return PS_OK;
}

// the splits of the cell axis: a function of M and N only, so that the order of the sums never depends on the data
static int64_t mod_split(int64_t npair, int64_t pitch) {
  const int64_t nchunk = (pitch + PS_MOD_KC - 1) / PS_MOD_KC;
  return std::max<int64_t>(1, std::min<int64_t>(nchunk, PS_MOD_BLOCKS / npair));
}

extern "C" int ps_modes_table(ps_modes* a, int slot, int centred, int64_t members_expected, double* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "modes_table: bad arguments");
  PS_TRY(mod_check_slot(a, slot, "modes_table"));
  if (members_expected != a->members)
    return ps_fail(PS_ERR_BAD_ARG, "modes_table: %lld members expected, the handle holds %lld",
                   (long long)members_expected, (long long)a->members);
  const int64_t M = a->members;
  const int64_t ntile = (M + PS_MOD_TILE - 1) / PS_MOD_TILE;
  const int64_t npair = ntile * (ntile + 1) / 2;
  if (npair > 0x7fffffffLL)
    return ps_fail(PS_ERR_BAD_ARG, "modes_table: %lld members are too many for one launch", (long long)M);
  const int64_t split = mod_split(npair, a->pitch);
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(mod_scratch(a, &a->part, &a->part_cap, (split + 1) * M * M, "the partial tables"));
  double* tab = a->part + split * M * M;
  const bool windowed = a->use_window;
  if (centred || windowed)
    PS_TRY(mod_mean_dev(a, slot));
  else
    PS_TRY(a->last.wait(a->stream));
  const double* mu = a->mu + (int64_t)slot * a->pitch;
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(2, a->stream, &e1));
  if (windowed) {
    PS_HIP(hipMemsetAsync(a->win, 0xff, sizeof(uint32_t), a->stream));
    PS_HIP(hipMemsetAsync(a->win + 1, 0, sizeof(uint32_t), a->stream));
    const int64_t nblk = std::min<int64_t>(1024, (a->pitch + PS_MOD_THREADS - 1) / PS_MOD_THREADS);
    hipLaunchKernelGGL(k_modes_window, dim3((unsigned)nblk), dim3(PS_MOD_THREADS), 0, a->stream, mu, a->pitch, a->win);
    PS_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_modes_gram, dim3((unsigned)npair, (unsigned)split), dim3(PS_MOD_THREADS), 0, a->stream,
                     a->X + (int64_t)slot * a->pitch, mod_member_doubles(a), centred ? mu : (const double*)nullptr, M,
                     (int)ntile, a->win, windowed ? (int64_t)0 : (a->pitch >> 6), a->pitch, a->part);
  PS_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_modes_reduce, dim3((unsigned)((M * M + PS_MOD_THREADS - 1) / PS_MOD_THREADS)),
                     dim3(PS_MOD_THREADS), 0, a->stream, a->part, M * M, (int)split, tab);
  PS_HIP(hipGetLastError());
  PS_TRY(a->prof.end(a->stream, e1));
  PS_TRY(a->last.mark(a->stream));
  PS_HIP(hipMemcpyAsync(out, tab, (size_t)(M * M) * sizeof(double), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  return PS_OK;
}

extern "C" int ps_modes_combine(ps_modes* a, int slot, int centred, int ncoef, const double* coef, double* out) {
  if (!a || !coef || !out) return ps_fail(PS_ERR_BAD_ARG, "modes_combine: bad arguments");
  PS_TRY(mod_check_slot(a, slot, "modes_combine"));
  if (ncoef < 1 || ncoef > PS_MOD_MAX_COEF)
    return ps_fail(PS_ERR_BAD_ARG, "modes_combine: %d coefficient rows (1..%d)", ncoef, PS_MOD_MAX_COEF);
  const int64_t M = a->members;
  PS_HIP(hipSetDevice(a->device));
  if (!a->maps)
    PS_TRY(mod_alloc((void**)&a->maps, (double)PS_MOD_MAX_COEF * a->pitch * sizeof(double), "modes_combine", "the maps"));
  if (centred)
    PS_TRY(mod_mean_dev(a, slot));
  else
    PS_TRY(a->last.wait(a->stream));
  PS_TRY(mod_weights_dev(a, (int64_t)PS_MOD_MAX_COEF * M));   // after the mean: a regrown block loses the weights
  double* cdev = a->wdev + M;
  PS_HIP(hipMemcpyAsync(cdev, coef, (size_t)(ncoef * M) * sizeof(double), hipMemcpyHostToDevice, a->stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(3, a->stream, &e1));
  const unsigned nblk = (unsigned)((a->pitch + PS_MOD_THREADS - 1) / PS_MOD_THREADS);
  hipLaunchKernelGGL(k_modes_combine, dim3(nblk), dim3(PS_MOD_THREADS), 0, a->stream, a->X + (int64_t)slot * a->pitch,
                     mod_member_doubles(a), centred ? a->mu + (int64_t)slot * a->pitch : (const double*)nullptr, M, cdev,
                     ncoef, a->pitch, a->maps);
  PS_HIP(hipGetLastError());
  PS_TRY(a->prof.end(a->stream, e1));
  PS_TRY(a->last.mark(a->stream));
  for (int k = 0; k < ncoef; ++k)
    PS_HIP(hipMemcpyAsync(out + (int64_t)k * a->ncell, a->maps + (int64_t)k * a->pitch, (size_t)a->ncell * sizeof(double),
                          hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));   // the coefficients are read until here
  return PS_OK;
}

extern "C" int ps_modes_fetch_member(ps_modes* a, int64_t member, int slot, double* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "modes_fetch_member: bad arguments");
  PS_TRY(mod_check_slot(a, slot, "modes_fetch_member"));
  if (member < 0 || member >= a->members)
    return ps_fail(PS_ERR_BAD_ARG, "modes_fetch_member: member %lld of %lld", (long long)member, (long long)a->members);
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  PS_HIP(hipMemcpyAsync(out, a->X + member * mod_member_doubles(a) + (int64_t)slot * a->pitch,
                        (size_t)a->ncell * sizeof(double), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  return PS_OK;
}

extern "C" int ps_modes_prof(ps_modes* a, int enable, double* ms, int64_t* launches) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "modes_prof: null handle");
  PS_HIP(hipSetDevice(a->device));
  a->prof.set(enable);
  if (!ms && !launches) return PS_OK;
  for (int k = 0; k < 4; ++k) PS_TRY(a->prof.totals(k, ms ? ms + k : nullptr, launches ? launches + k : nullptr));
  return PS_OK;
}
