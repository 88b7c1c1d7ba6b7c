// Core-range maps (include/parasitoid_hip.h, ps_range_*): per fraction p_j and slot the weighted count of the
// members whose smallest region holding the share p_j of their own mass -- the highest-density region
// {v >= lambda_j}, the isopleth of the utilisation distribution -- contains the cell, and per member the level
// lambda_j, the cells n_j of the region, the integer mass Q and its exponent E.  The value of a slot is the one
// ps_summary_add adds (ps_record_value).  Layout (pitch = N*N rounded up to 64 cells, as ps_summary.hip):
//   cnt[j][slot][pitch]       uint32, the weight of the members with v >= lambda_j
//   lam[member][j][slot]      fp64,   n[member][j][slot] uint32
//   Q[member][slot]           uint64, E[member][slot]    int32         (grow by doubling, as ps_arrival's rows)
//   st                        the pass scratch of the member being added (RangeState)
// One add: k_range_max (the largest bit pattern, an integer max), then RNG_PASSES times k_range_hist (the integer
// mass per digit among the cells that match each fraction's prefix, uint64 adds in LDS folded to global memory)
// and k_range_pick (extends every (slot, fraction) prefix by the digit at which the mass from above reaches the
// needed mass), then k_range_count (one writer per cell; n by ballots and one integer atomic per block).  All
// slots of a member go through each launch (slot on grid.y).  The select runs on key = bits(v) - bits(2^(E-36)):
// positive doubles order as their bit patterns, cells below 2^(E-36) have mass 0 and cannot hold the level, and
// the key is < 37 * 2^52 < 2^60.  Integer atomics only: neither the order of adds nor that of merges nor the grid
// changes a bit.
#include <math.h>
#include <stddef.h>

#include <algorithm>
#include <vector>

#include "ps_common.h"

#define PS_RNG_MAX_SLOT 32   // one launch's descriptors: 32 x 32 B of kernel arguments
#define PS_RNG_MAX_FRAC 4
#define PS_RNG_THREADS 256
#define PS_RNG_ROWS0 64      // member rows allocated at create
#define RNG_BITS 10          // digit width of one select pass
#define RNG_BINS (1 << RNG_BITS)
#define RNG_PASSES 6         // 60 key bits
#define RNG_CHUNK 16         // cells per thread of k_range_hist: one block zeroes and folds its bins once per 4096 cells
#define RNG_INF_BITS 0x7ff0000000000000ull

namespace {

struct RngSlots {
  PsSrc s[PS_RNG_MAX_SLOT];
};
// p_j = m * 2^-k exactly, m the 53-bit significand
struct RngFrac {
  uint64_t m[PS_RNG_MAX_FRAC];
  int k[PS_RNG_MAX_FRAC];
};

// the pass scratch of one member, zeroed at the start of every add
struct RangeState {
  uint64_t vmax[PS_RNG_MAX_SLOT];                       // the largest bit pattern of a value > 0, 0: empty slot
  uint64_t need[PS_RNG_MAX_SLOT][PS_RNG_MAX_FRAC];
  uint64_t above[PS_RNG_MAX_SLOT][PS_RNG_MAX_FRAC];     // the mass of the keys above the prefix's range
  uint64_t prefix[PS_RNG_MAX_SLOT][PS_RNG_MAX_FRAC];
  uint64_t lam[PS_RNG_MAX_SLOT][PS_RNG_MAX_FRAC];       // the level's bit pattern, once the last pass picked
  uint64_t hist[PS_RNG_MAX_SLOT][PS_RNG_MAX_FRAC][RNG_BINS];
};

__device__ inline double rng_value(const PsSrc& sd, int64_t i, double negval) {
  const double delta = sd.stats ? sd.stats->delta : 0.0;
  return ps_record_value(sd.rec[i], sd.stat_scale, sd.post_scale, delta, negval);
}
// the bit pattern of a finite value > 0, else 0 (a cell that is not > 0, or not finite, has no mass and lies in no set)
__device__ inline uint64_t rng_bits(double v) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return v > 0.0 && b < RNG_INF_BITS ? b : 0ull;
}
// E = floor(log2 vmax) from the exponent field; a subnormal maximum from its leading bit
__device__ inline int rng_exponent(uint64_t vb) {
  const int be = (int)(vb >> 52);
  return be > 0 ? be - 1023 : 63 - __clzll((long long)vb) - 1074;
}
// the pattern of 2^(E - 36), the smallest value with mass >= 1 (0 where it underflows: every value > 0 has mass)
__device__ inline uint64_t rng_base(int E) { return (uint64_t)__double_as_longlong(ldexp(1.0, E - 36)); }
// the smallest integer >= m * 2^-k * Q, k >= 1, by the 128-bit product
__device__ inline uint64_t rng_need(uint64_t m, int k, uint64_t Q) {
  const uint64_t lo = m * Q, hi = __umul64hi(m, Q);
  uint64_t q, rem;
  if (k >= 128) {
    q = 0;
    rem = hi | lo;
  } else if (k >= 64) {
    const int r = k - 64;
    q = hi >> r;
    rem = (hi & ((1ull << r) - 1)) | lo;
  } else {
    q = (hi << (64 - k)) | (lo >> k);
    rem = lo & ((1ull << k) - 1);
  }
  return q + (rem != 0);
}

// slot on grid.y, a block takes RNG_CHUNK * 256 cells: the largest pattern of each wave by shuffles, and one integer
// atomic per wave only where it would raise the slot's maximum as it stands (it only grows, so a stale read costs
// at most a needless atomic).  Ten thousand waves per slot updating one address took 1 ms at R = 400.
__global__ void __launch_bounds__(PS_RNG_THREADS) k_range_max(RngSlots desc, RangeState* __restrict__ st, int64_t ncell,
                                                              double negval) {
  const int s = blockIdx.y;
  const int64_t i0 = blockIdx.x * (int64_t)(RNG_CHUNK * PS_RNG_THREADS) + threadIdx.x;
  uint64_t b = 0;
  for (int it = 0; it < RNG_CHUNK; ++it) {
    const int64_t i = i0 + (int64_t)it * PS_RNG_THREADS;
    if (i >= ncell) break;
    const uint64_t x = rng_bits(rng_value(desc.s[s], i, negval));
    b = x > b ? x : b;
  }
  if (!__any(b != 0)) return;
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t o = __shfl_xor(b, off);
    b = o > b ? o : b;
  }
  if ((threadIdx.x & 63) == 0) {
    unsigned long long* at = (unsigned long long*)&st->vmax[s];
    if (b > __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(at, (unsigned long long)b);
  }
}

// pass `pass` of the select: hist[s][j][digit] += q over the cells whose key matches prefix[s][j]; in pass 0 every
// prefix is empty and fraction 0's bins serve all.  A block takes RNG_CHUNK * 256 cells; bins no cell of the block
// touched cost no global atomic.
__global__ void __launch_bounds__(PS_RNG_THREADS) k_range_hist(RngSlots desc, RangeState* __restrict__ st, int pass,
                                                               int nfrac, int64_t ncell, double negval) {
  extern __shared__ uint64_t bins[];   // [nf][RNG_BINS]
  const int s = blockIdx.y;
  const uint64_t vb = st->vmax[s];
  if (vb == 0) return;   // empty slot: the whole block leaves
  const int nf = pass == 0 ? 1 : nfrac;
  for (int t = threadIdx.x; t < nf * RNG_BINS; t += blockDim.x) bins[t] = 0;
  const int E = rng_exponent(vb);
  const uint64_t base = rng_base(E);
  uint64_t prefix[PS_RNG_MAX_FRAC];
#pragma unroll
  for (int j = 0; j < PS_RNG_MAX_FRAC; ++j) prefix[j] = j < nf ? st->prefix[s][j] : 0;
  const int hi_shift = RNG_BITS * (RNG_PASSES - pass), lo_shift = hi_shift - RNG_BITS;
  __syncthreads();
  int touched = 0;
  const int64_t i0 = blockIdx.x * (int64_t)(RNG_CHUNK * PS_RNG_THREADS) + threadIdx.x;
  for (int it = 0; it < RNG_CHUNK; ++it) {
    const int64_t i = i0 + (int64_t)it * PS_RNG_THREADS;
    if (i >= ncell) break;
    const double v = rng_value(desc.s[s], i, negval);
    const uint64_t b = rng_bits(v);
    if (b == 0 || b < base) continue;
    const uint64_t key = b - base;
    const uint64_t q = (uint64_t)ldexp(v, 36 - E);   // exact scaling, truncation = floor
    const uint64_t head = hi_shift < 64 ? key >> hi_shift : 0ull;
    const int digit = (int)((key >> lo_shift) & (RNG_BINS - 1));
#pragma unroll
    for (int j = 0; j < PS_RNG_MAX_FRAC; ++j) {
      if (j < nf && head == prefix[j]) {
        atomicAdd((unsigned long long*)&bins[j * RNG_BINS + digit], (unsigned long long)q);
        touched = 1;
      }
    }
  }
  if (!__syncthreads_or(touched)) return;
  for (int t = threadIdx.x; t < nf * RNG_BINS; t += blockDim.x) {
    const uint64_t h = bins[t];
    if (h) atomicAdd((unsigned long long*)&st->hist[s][t / RNG_BINS][t % RNG_BINS], (unsigned long long)h);
  }
}

// block s, RNG_BINS threads: every fraction's prefix takes the largest digit d at which above + the mass of the
// digits >= d reaches the need; pass 0 first forms Q (the sum of all bins) and the needs; the last pass writes the
// member's level and zeroes its cell count.  The bins are left zeroed for the next pass.
__global__ void __launch_bounds__(RNG_BINS) k_range_pick(RangeState* __restrict__ st, int pass, int nslot, int nfrac,
                                                         RngFrac frac, double* __restrict__ lam, uint32_t* __restrict__ n,
                                                         uint64_t* __restrict__ Qrow, int32_t* __restrict__ Erow) {
  __shared__ uint64_t sc[RNG_BINS];
  const int s = blockIdx.x, t = threadIdx.x;
  const uint64_t vb = st->vmax[s];
  const int E = vb ? rng_exponent(vb) : 0;
  for (int j = 0; j < nfrac; ++j) {
    const int hj = pass == 0 ? 0 : j;
    // the state of (s, j) before the barrier: the thread that picks writes it while the others may still compare
    uint64_t need = pass ? st->need[s][j] : 0, above = pass ? st->above[s][j] : 0, prefix = pass ? st->prefix[s][j] : 0;
    sc[t] = st->hist[s][hj][t];
    __syncthreads();
    for (int off = 1; off < RNG_BINS; off <<= 1) {   // sc[t] = the mass of the digits >= t
      const uint64_t x = t + off < RNG_BINS ? sc[t + off] : 0ull;
      __syncthreads();
      sc[t] += x;
      __syncthreads();
    }
    if (pass == 0) {
      const uint64_t Q = sc[0];
      need = rng_need(frac.m[j], frac.k[j], Q);
      if (t == 0) {
        st->need[s][j] = need;
        if (j == 0) {
          Qrow[s] = Q;
          Erow[s] = E;
        }
      }
    }
    const uint64_t mine = above + sc[t], next = t + 1 < RNG_BINS ? sc[t + 1] : 0ull;
    if (mine >= need && (t + 1 == RNG_BINS || above + next < need)) {   // exactly one thread: sc does not increase in t
      prefix = (prefix << RNG_BITS) | (uint64_t)t;
      st->prefix[s][j] = prefix;
      st->above[s][j] = above + next;
      if (pass == RNG_PASSES - 1) {
        const uint64_t lb = vb ? prefix + rng_base(E) : RNG_INF_BITS;
        st->lam[s][j] = lb;
        lam[j * nslot + s] = __longlong_as_double((long long)lb);
        n[j * nslot + s] = 0;
      }
    }
    __syncthreads();
  }
  const int nf = pass == 0 ? 1 : nfrac;
  for (int j = 0; j < nf; ++j) st->hist[s][j][t] = 0;
}

// slot on grid.y, a block takes RNG_CHUNK * 256 cells, one writer per cell: C_j += w where v >= lambda_j; n_j by a
// ballot per wave and step carried in a register, one LDS atomic per wave and one global integer atomic per block
// and fraction.  A wave outside the widest set only loads.
__global__ void __launch_bounds__(PS_RNG_THREADS) k_range_count(RngSlots desc, const RangeState* __restrict__ st,
                                                                int nslot, int nfrac, uint32_t* __restrict__ cnt,
                                                                uint32_t* __restrict__ n, int64_t ncell, int64_t pitch,
                                                                double negval, uint32_t w) {
  __shared__ uint32_t tot[PS_RNG_MAX_FRAC];
  const int s = blockIdx.y;
  if (st->vmax[s] == 0) return;   // empty slot: the whole block leaves
  if (threadIdx.x < PS_RNG_MAX_FRAC) tot[threadIdx.x] = 0;
  uint64_t lam[PS_RNG_MAX_FRAC];
  uint32_t mine[PS_RNG_MAX_FRAC];
#pragma unroll
  for (int j = 0; j < PS_RNG_MAX_FRAC; ++j) {
    lam[j] = st->lam[s][j < nfrac ? j : nfrac - 1];
    mine[j] = 0;
  }
  const uint64_t widest = st->lam[s][nfrac - 1];
  __syncthreads();
  const int64_t i0 = blockIdx.x * (int64_t)(RNG_CHUNK * PS_RNG_THREADS) + threadIdx.x;
  for (int it = 0; it < RNG_CHUNK; ++it) {
    const int64_t i = i0 + (int64_t)it * PS_RNG_THREADS;
    const uint64_t b = i < ncell ? rng_bits(rng_value(desc.s[s], i, negval)) : 0ull;
    if (!__any(b != 0 && b >= widest)) continue;
#pragma unroll
    for (int j = 0; j < PS_RNG_MAX_FRAC; ++j) {
      if (j < nfrac) {
        const bool in = b != 0 && b >= lam[j];
        if (in) cnt[((int64_t)j * nslot + s) * pitch + i] += w;
        mine[j] += (uint32_t)__popcll(__ballot(in));   // the same in every lane
      }
    }
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < PS_RNG_MAX_FRAC; ++j)
      if (j < nfrac && mine[j]) atomicAdd(&tot[j], mine[j]);
  }
  __syncthreads();
  if ((int)threadIdx.x < nfrac && tot[threadIdx.x]) atomicAdd(&n[threadIdx.x * nslot + s], tot[threadIdx.x]);
}

// flat over nfrac * nslot * pitch words
__global__ void k_range_merge(uint32_t* __restrict__ ca, const uint32_t* __restrict__ cb, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) ca[i] += cb[i];
}

__global__ void k_range_prob(const uint32_t* __restrict__ c, int64_t ncell, double W, double* __restrict__ prob) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < ncell) prob[i] = (double)c[i] / W;
}

}  // namespace

struct ps_range {
  int device = 0, N = 0, nslot = 0, nfrac = 0;
  std::vector<double> frac;
  RngFrac fr;
  int64_t ncell = 0, pitch = 0;
  uint32_t* cnt = nullptr;     // [j][slot][pitch]
  RangeState* st = nullptr;
  double* lam = nullptr;       // [rows_cap][j][slot]
  uint32_t* n = nullptr;       // [rows_cap][j][slot]
  uint64_t* Q = nullptr;       // [rows_cap][slot]
  int32_t* E = nullptr;        // [rows_cap][slot]
  int64_t rows_cap = 0;
  double* map = nullptr;       // [pitch] map scratch
  uint64_t W = 0;
  int64_t members = 0;
  std::vector<uint32_t> weights;   // per member, in row order
  hipStream_t stream = nullptr;    // reset / merge / maps / fetch / row growth
  PsLastOp last;                   // the last operation, on whatever stream it ran
  PsProf prof;                     // channel 0: the adds, 1: the maps
};

static int64_t rng_row_len(const ps_range* a) { return (int64_t)a->nfrac * a->nslot; }
static size_t rng_cnt_bytes(const ps_range* a) { return (size_t)rng_row_len(a) * a->pitch * sizeof(uint32_t); }
// one member's rows: lambda 8 B + n 4 B per (fraction, slot), Q 8 B + E 4 B per slot
static size_t rng_member_bytes(const ps_range* a) { return (size_t)rng_row_len(a) * 12 + (size_t)a->nslot * 12; }

// hipMalloc behind a check against the free device memory: PS_ERR_OOM before anything is allocated
static int rng_alloc(void** p, size_t bytes, const char* what) {
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (bytes > free_b)
    return ps_fail(PS_ERR_OOM, "range: %s needs %.3g GB, %.3g GB free", what, (double)bytes * 1e-9, (double)free_b * 1e-9);
  PS_HIP(hipMalloc(p, bytes));
  return PS_OK;
}

// room for `need` member rows: a doubling copies the rows so far on the handle's stream and synchronises once
// before the old blocks are freed
static int rng_reserve_rows(ps_range* a, int64_t need) {
  if (need <= a->rows_cap) return PS_OK;
  int64_t cap = std::max<int64_t>(a->rows_cap, PS_RNG_ROWS0);
  while (cap < need) cap *= 2;
  const size_t nks = (size_t)rng_row_len(a), ns = (size_t)a->nslot;
  const size_t row_b[4] = {nks * sizeof(double), nks * sizeof(uint32_t), ns * sizeof(uint64_t), ns * sizeof(int32_t)};
  void* old[4] = {a->lam, a->n, a->Q, a->E};
  void* p[4] = {nullptr, nullptr, nullptr, nullptr};
  auto drop = [&]() {
    for (void* q : p)
      if (q) (void)hipFree(q);
  };
  for (int t = 0; t < 4; ++t) {
    const int rc = rng_alloc(&p[t], (size_t)cap * row_b[t], "the member rows");
    if (rc != PS_OK) {
      drop();
      return rc;
    }
  }
  if (a->rows_cap > 0) {
    hipError_t e = hipSuccess;
    if (a->last.live) e = hipStreamWaitEvent(a->stream, a->last.ev, 0);
    for (int t = 0; t < 4 && e == hipSuccess && a->members > 0; ++t)
      e = hipMemcpyAsync(p[t], old[t], (size_t)a->members * row_b[t], hipMemcpyDeviceToDevice, a->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(a->stream);
    if (e != hipSuccess) {
      drop();
      return ps_fail(PS_ERR_HIP, "range: growing the member rows: %s", hipGetErrorString(e));
    }
    for (void* q : old) PS_HIP(hipFree(q));
  }
  a->lam = (double*)p[0];
  a->n = (uint32_t*)p[1];
  a->Q = (uint64_t*)p[2];
  a->E = (int32_t*)p[3];
  a->rows_cap = cap;
  return PS_OK;
}

extern "C" void ps_range_destroy(ps_range* a) {
  if (!a) return;
  (void)hipSetDevice(a->device);
  a->last.sync();
  if (a->stream) (void)hipStreamSynchronize(a->stream);
  a->prof.release();
  for (void* p : {(void*)a->cnt, (void*)a->st, (void*)a->lam, (void*)a->n, (void*)a->Q, (void*)a->E, (void*)a->map})
    if (p) (void)hipFree(p);
  a->last.destroy();
  if (a->stream) (void)hipStreamDestroy(a->stream);
  delete a;
}

extern "C" int ps_range_reset(ps_range* a) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "range_reset: null handle");
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  PS_HIP(hipMemsetAsync(a->cnt, 0, rng_cnt_bytes(a), a->stream));
  PS_HIP(hipMemsetAsync(a->st, 0, sizeof(RangeState), a->stream));
  PS_TRY(a->last.mark(a->stream));
  a->W = 0;
  a->members = 0;
  a->weights.clear();
  if (!a->prof.idle()) PS_HIP(hipStreamSynchronize(a->stream));
  a->prof.release();   // the timings so far go with the members
  return PS_OK;
}

extern "C" int ps_range_create(int device, int N, int nslot, int nfrac, const double* frac, ps_range** out) {
  if (!out || N < 1 || nslot < 1 || nslot > PS_RNG_MAX_SLOT || nfrac < 1 || nfrac > PS_RNG_MAX_FRAC || !frac)
    return ps_fail(PS_ERR_BAD_ARG, "range_create: N %d, %d slots (1..%d), %d fractions (1..%d)", N, nslot,
                   PS_RNG_MAX_SLOT, nfrac, PS_RNG_MAX_FRAC);
  *out = nullptr;
  for (int j = 0; j < nfrac; ++j) {
    if (!(frac[j] > 0.0 && frac[j] < 1.0))
      return ps_fail(PS_ERR_BAD_ARG, "range_create: fraction %d = %g is not in (0, 1)", j, frac[j]);
    if (j > 0 && !(frac[j] > frac[j - 1]))
      return ps_fail(PS_ERR_BAD_ARG, "range_create: fractions not strictly increasing at %d", j);
  }
  const int64_t ncell = (int64_t)N * N;
  if (ncell >= (1ll << 25))
    return ps_fail(PS_ERR_BAD_ARG, "range_create: N %d: the integer mass needs N * N < 2^25", N);
  PS_TRY(ps_use_device(device));
  const int64_t pitch = (ncell + 63) / 64 * 64;
  ps_range* a = new ps_range();
  a->device = device;
  a->N = N;
  a->nslot = nslot;
  a->nfrac = nfrac;
  a->frac.assign(frac, frac + nfrac);
  for (int j = 0; j < PS_RNG_MAX_FRAC; ++j) {
    a->fr.m[j] = 0;
    a->fr.k[j] = 1;
    if (j < nfrac) {
      int e = 0;
      const double f = frexp(frac[j], &e);   // frac = f * 2^e, f in [0.5, 1), e <= 0
      a->fr.m[j] = (uint64_t)ldexp(f, 53);
      a->fr.k[j] = 53 - e;
    }
  }
  a->ncell = ncell;
  a->pitch = pitch;
  auto fail = [&](int rc) {
    ps_range_destroy(a);
    return rc;
  };
  hipError_t e = hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = a->last.create();
  if (e != hipSuccess) return fail(ps_fail(PS_ERR_HIP, "range_create: %s", hipGetErrorString(e)));
  int rc = rng_alloc((void**)&a->cnt, rng_cnt_bytes(a), "the count planes");
  if (rc == PS_OK) rc = rng_alloc((void**)&a->st, sizeof(RangeState), "the pass scratch");
  if (rc == PS_OK) rc = rng_alloc((void**)&a->map, (size_t)pitch * sizeof(double), "the map scratch");
  if (rc == PS_OK) rc = rng_reserve_rows(a, PS_RNG_ROWS0);
  if (rc == PS_OK) rc = ps_range_reset(a);
  if (rc != PS_OK) return fail(rc);
  *out = a;
  return PS_OK;
}

extern "C" int ps_range_reserve(ps_range* a, int64_t members) {
  if (!a || members < 0) return ps_fail(PS_ERR_BAD_ARG, "range_reserve: bad arguments");
  PS_HIP(hipSetDevice(a->device));
  return rng_reserve_rows(a, members);
}

// one member from the slot descriptors (one per slot of the handle, the rest null), enqueued on `stream`
static int rng_launch(ps_range* a, const RngSlots& desc, hipStream_t stream, double negval, uint32_t weight) {
  PS_TRY(rng_reserve_rows(a, a->members + 1));
  PS_TRY(a->last.wait(stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(0, stream, &e1));
  const int64_t nks = rng_row_len(a);
  double* lam = a->lam + a->members * nks;
  uint32_t* n = a->n + a->members * nks;
  const int64_t per_blk = (int64_t)RNG_CHUNK * PS_RNG_THREADS;
  const unsigned nbh = (unsigned)((a->ncell + per_blk - 1) / per_blk);
  PS_HIP(hipMemsetAsync(a->st, 0, offsetof(RangeState, hist), stream));   // k_range_pick leaves the bins zeroed
  hipLaunchKernelGGL(k_range_max, dim3(nbh, a->nslot), dim3(PS_RNG_THREADS), 0, stream, desc, a->st, a->ncell, negval);
  PS_HIP(hipGetLastError());
  for (int pass = 0; pass < RNG_PASSES; ++pass) {
    const size_t lds = (size_t)(pass == 0 ? 1 : a->nfrac) * RNG_BINS * sizeof(uint64_t);
    hipLaunchKernelGGL(k_range_hist, dim3(nbh, a->nslot), dim3(PS_RNG_THREADS), lds, stream, desc, a->st, pass,
                       a->nfrac, a->ncell, negval);
    PS_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_range_pick, dim3(a->nslot), dim3(RNG_BINS), 0, stream, a->st, pass, a->nslot, a->nfrac, a->fr,
                       lam, n, a->Q + a->members * a->nslot, a->E + a->members * a->nslot);
    PS_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_range_count, dim3(nbh, a->nslot), dim3(PS_RNG_THREADS), 0, stream, desc, a->st, a->nslot,
                     a->nfrac, a->cnt, n, a->ncell, a->pitch, negval, weight);
  PS_HIP(hipGetLastError());
  PS_TRY(a->prof.end(stream, e1));
  PS_TRY(a->last.mark(stream));
  a->W += weight;
  a->members += 1;
  a->weights.push_back(weight);
  return PS_OK;
}

extern "C" int ps_range_add(ps_range* a, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                            const double* stat_scale, const double* post_scale, const int32_t* use_delta,
                            double negval, uint32_t weight) {
  if (!a || !s || !kind || !idx || !stat_scale || !post_scale || !use_delta)
    return ps_fail(PS_ERR_BAD_ARG, "range_add: bad arguments");
  if (nslot != a->nslot) return ps_fail(PS_ERR_BAD_ARG, "range_add: %d slots given, the handle has %d", nslot, a->nslot);
  if (weight < 1) return ps_fail(PS_ERR_BAD_ARG, "range_add: weight must be >= 1");
  if (a->W + weight > 0xffffffffull)
    return ps_fail(PS_ERR_BAD_ARG, "range_add: total weight %llu would overflow the uint32 counts",
                   (unsigned long long)(a->W + weight));
  PS_HIP(hipSetDevice(a->device));
  // every descriptor first: an add with a bad slot enqueues nothing
  RngSlots desc;
  hipStream_t stream = nullptr;
  PS_TRY(ps_read_records("range_add", "handle", a->device, a->N, s, nslot, kind, idx, stat_scale, post_scale, use_delta,
                         false, desc.s, &stream));
  for (int i = nslot; i < PS_RNG_MAX_SLOT; ++i) desc.s[i] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  return rng_launch(a, desc, stream, negval, weight);
}

// one member whose slots are the current fields of a projection or a release plan, in ascending output order
// (who: the entry point)
static int rng_add_fields(ps_range* a, void* h, const PsFieldsOps& src, const char* who, uint32_t weight) {
  if (!a || !h) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  if (weight < 1) return ps_fail(PS_ERR_BAD_ARG, "%s: weight must be >= 1", who);
  if (a->W + weight > 0xffffffffull)
    return ps_fail(PS_ERR_BAD_ARG, "%s: total weight %llu would overflow the uint32 counts", who,
                   (unsigned long long)(a->W + weight));
  // slot e takes Y_e: no statistics, both scales 1 and negval 0, so the value rule returns Y itself
  RngSlots desc;
  PS_TRY(ps_read_fields(who, "handle", "slots", a->device, a->N, a->nslot, h, src, desc.s));
  for (int e = a->nslot; e < PS_RNG_MAX_SLOT; ++e) desc.s[e] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(src.wait(h, a->stream));
  PS_TRY(rng_launch(a, desc, a->stream, 0.0, weight));
  return src.mark(h, a->stream);   // the next apply overwrites Y only after this read
}

extern "C" int ps_range_add_project(ps_range* a, ps_project* p, uint32_t weight) {
  return rng_add_fields(a, p, ps_project_fields(), "range_add_project", weight);
}

extern "C" int ps_range_add_sites(ps_range* a, ps_sites* p, uint32_t weight) {
  return rng_add_fields(a, p, ps_sites_fields(), "range_add_sites", weight);
}

extern "C" int ps_range_merge(ps_range* dst, ps_range* src) {
  if (!dst || !src || dst == src) return ps_fail(PS_ERR_BAD_ARG, "range_merge: bad arguments");
  if (dst->device != src->device || dst->N != src->N || dst->nslot != src->nslot || dst->frac != src->frac)
    return ps_fail(PS_ERR_BAD_ARG, "range_merge: handles differ in device, domain, slots or fractions");
  if (dst->W + src->W > 0xffffffffull) return ps_fail(PS_ERR_BAD_ARG, "range_merge: total weight would overflow");
  if (src->members == 0) return PS_OK;
  PS_HIP(hipSetDevice(dst->device));
  PS_TRY(rng_reserve_rows(dst, dst->members + src->members));
  PS_TRY(dst->last.wait(dst->stream));
  PS_TRY(src->last.wait(dst->stream));
  hipLaunchKernelGGL(k_range_merge, dim3(2048), dim3(256), 0, dst->stream, dst->cnt, src->cnt,
                     rng_row_len(dst) * dst->pitch);
  PS_HIP(hipGetLastError());
  const int64_t nks = rng_row_len(dst), ns = dst->nslot, m0 = dst->members, m1 = src->members;
  PS_HIP(hipMemcpyAsync(dst->lam + m0 * nks, src->lam, (size_t)(m1 * nks) * sizeof(double), hipMemcpyDeviceToDevice,
                        dst->stream));
  PS_HIP(hipMemcpyAsync(dst->n + m0 * nks, src->n, (size_t)(m1 * nks) * sizeof(uint32_t), hipMemcpyDeviceToDevice,
                        dst->stream));
  PS_HIP(hipMemcpyAsync(dst->Q + m0 * ns, src->Q, (size_t)(m1 * ns) * sizeof(uint64_t), hipMemcpyDeviceToDevice,
                        dst->stream));
  PS_HIP(hipMemcpyAsync(dst->E + m0 * ns, src->E, (size_t)(m1 * ns) * sizeof(int32_t), hipMemcpyDeviceToDevice,
                        dst->stream));
  PS_TRY(dst->last.mark(dst->stream));
  PS_TRY(src->last.mark(dst->stream));   // src is read until then
  dst->W += src->W;
  dst->members += src->members;
  dst->weights.insert(dst->weights.end(), src->weights.begin(), src->weights.end());
  return PS_OK;
}

extern "C" int ps_range_info(ps_range* a, double* total_weight, int64_t* members, int64_t* capacity, int64_t* bytes) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "range_info: null handle");
  if (total_weight) *total_weight = (double)a->W;
  if (members) *members = a->members;
  if (capacity) *capacity = a->rows_cap;
  if (bytes)
    *bytes = (int64_t)(rng_cnt_bytes(a) + sizeof(RangeState) + (size_t)a->pitch * sizeof(double) +
                       (size_t)a->rows_cap * rng_member_bytes(a));
  return PS_OK;
}

static int rng_check(ps_range* a, int j, int slot, const char* who) {
  if (j < 0 || j >= a->nfrac) return ps_fail(PS_ERR_BAD_ARG, "%s: fraction %d of %d", who, j, a->nfrac);
  if (slot < 0 || slot >= a->nslot) return ps_fail(PS_ERR_BAD_ARG, "%s: slot %d of %d", who, slot, a->nslot);
  if (a->W == 0) return ps_fail(PS_ERR_STATE, "%s: nothing accumulated (W = 0)", who);
  return PS_OK;
}

extern "C" int ps_range_prob(ps_range* a, int j, int slot, double* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "range_prob: bad arguments");
  PS_TRY(rng_check(a, j, slot, "range_prob"));
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(a->prof.begin(1, a->stream, &e1));
  const uint32_t* c = a->cnt + ((int64_t)j * a->nslot + slot) * a->pitch;
  hipLaunchKernelGGL(k_range_prob, dim3((unsigned)((a->ncell + 255) / 256)), dim3(256), 0, a->stream, c, a->ncell,
                     (double)a->W, a->map);
  PS_HIP(hipGetLastError());
  PS_TRY(a->prof.end(a->stream, e1));
  PS_TRY(a->last.mark(a->stream));
  PS_HIP(hipMemcpyAsync(out, a->map, (size_t)a->ncell * sizeof(double), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  return PS_OK;
}

extern "C" int ps_range_fetch_counts(ps_range* a, int j, int slot, uint32_t* out) {
  if (!a || !out) return ps_fail(PS_ERR_BAD_ARG, "range_fetch_counts: bad arguments");
  PS_TRY(rng_check(a, j, slot, "range_fetch_counts"));
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  const uint32_t* src = a->cnt + ((int64_t)j * a->nslot + slot) * a->pitch;
  PS_HIP(hipMemcpyAsync(out, src, (size_t)a->ncell * sizeof(uint32_t), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  return PS_OK;
}

extern "C" int ps_range_fetch_members(ps_range* a, int j, int slot, double* lambda, uint32_t* cells, uint32_t* weights) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "range_fetch_members: null handle");
  PS_TRY(rng_check(a, j, slot, "range_fetch_members"));
  const int64_t m = a->members, nks = rng_row_len(a), at = (int64_t)j * a->nslot + slot;
  if (weights)
    for (int64_t r = 0; r < m; ++r) weights[r] = a->weights[(size_t)r];
  if (!lambda && !cells) return PS_OK;
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  std::vector<double> hl;
  std::vector<uint32_t> hn;
  if (lambda) {
    hl.resize((size_t)(m * nks));
    PS_HIP(hipMemcpyAsync(hl.data(), a->lam, hl.size() * sizeof(double), hipMemcpyDeviceToHost, a->stream));
  }
  if (cells) {
    hn.resize((size_t)(m * nks));
    PS_HIP(hipMemcpyAsync(hn.data(), a->n, hn.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, a->stream));
  }
  PS_HIP(hipStreamSynchronize(a->stream));
  for (int64_t r = 0; r < m; ++r) {
    if (lambda) lambda[r] = hl[(size_t)(r * nks + at)];
    if (cells) cells[r] = hn[(size_t)(r * nks + at)];
  }
  return PS_OK;
}

extern "C" int ps_range_fetch_mass(ps_range* a, int slot, uint64_t* Q, int32_t* E) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "range_fetch_mass: null handle");
  PS_TRY(rng_check(a, 0, slot, "range_fetch_mass"));
  const int64_t m = a->members, ns = a->nslot;
  if (!Q && !E) return PS_OK;
  PS_HIP(hipSetDevice(a->device));
  PS_TRY(a->last.wait(a->stream));
  std::vector<uint64_t> hq((size_t)(m * ns));
  std::vector<int32_t> he((size_t)(m * ns));
  PS_HIP(hipMemcpyAsync(hq.data(), a->Q, hq.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipMemcpyAsync(he.data(), a->E, he.size() * sizeof(int32_t), hipMemcpyDeviceToHost, a->stream));
  PS_HIP(hipStreamSynchronize(a->stream));
  for (int64_t r = 0; r < m; ++r) {
    if (Q) Q[r] = hq[(size_t)(r * ns + slot)];
    if (E) E[r] = he[(size_t)(r * ns + slot)];
  }
  return PS_OK;
}

extern "C" int ps_range_prof(ps_range* a, int enable, double* add_ms, int64_t* adds, double* map_ms, int64_t* maps) {
  if (!a) return ps_fail(PS_ERR_BAD_ARG, "range_prof: null handle");
  PS_HIP(hipSetDevice(a->device));
  a->prof.set(enable);
  double* ms_out[2] = {add_ms, map_ms};
  int64_t* n_out[2] = {adds, maps};
  for (int k = 0; k < 2; ++k)
    if (ms_out[k] || n_out[k]) PS_TRY(a->prof.totals(k, ms_out[k], n_out[k]));
  return PS_OK;
}
