// Ranking of P named release plans or P projections, member by member (include/parasitoid_hip.h, ps_rank_*):
// with a_j the value plan j holds at a cell for one member and m = max_j a_j, per slot and cell the weight of
// the members in which plan j alone holds m (best_j; a tie counts for nobody), the weighted mean and M2 of the
// regret r_j = m - a_j, per threshold t_k the weight of the members in which plan j alone reaches t_k (sole_kj),
// some plan does (any_k) and every plan does (all_k), and per member the cells every plan covers at every
// threshold and slot.  All plans' fields belong to the same member, so the joint statements are kept.  Layout
// (pitch = N*N rounded up to 64 cells, as ps_summary.hip; Q = P + nthr (P + 2) count planes):
//   mean[slot][plan][pitch], m2[slot][plan][pitch]   fp64, the step of ps_summary.hip (sum_update) on r_j
//   cnt[slot][Q][pitch]                              uint32: best_0 .. best_{P-1}, then per k sole_k0 ..
//                                                    sole_k,P-1, any_k, all_k
//   rows[member][plan][k][slot]                      uint32, cells with a_j >= t_k; grows by doubling
// An add reads 16 B of every plan per cell pair and slot and reads + writes 16 B of a mean, 16 B of an M2 and
// 8 B of a count plane only where the pair changes something: most of the domain is 0 for every plan, a P-fold
// tie at regret 0 against a mean of 0.  The kernel is instantiated per P, so the P values of a cell pair are
// named registers (no scratch).  One thread owns a pair of cells, so every mean, M2 and count cell has a single
// writer; the per-member cell counts are popcounts of wave ballots carried in registers over the grid stride,
// summed over the block's waves in LDS, then one integer atomicAdd per block and counter.  No floating-point
// atomics: neither the order of adds nor that of merges nor the grid changes a bit of a count.
#include <math.h>

#include <algorithm>
#include <vector>

#include "ps_common.h"

#define PS_RANK_MIN_PLANS 2
#define PS_RANK_MAX_PLANS 8
#define PS_RANK_MAX_THR 4
#define PS_RANK_DESC_BYTES 1152   // of slot descriptors per launch: 16 slots at P = 8, 32 (the cap) at P <= 3
#define PS_RANK_MAX_CHUNK 32
#define PS_RANK_THREADS 256
#define PS_RANK_MAX_BLOCKS 4096   // per slot, as ps_summary.hip; more pairs than 4096 x 256 take the grid stride
#define PS_RANK_ROWS0 64          // member rows allocated at create

namespace {

template <int P>
struct RankSlot {
  const double* a[P];
  int slot;
};
template <int P>
constexpr int rank_chunk() {
  return std::min<int>(PS_RANK_MAX_CHUNK, PS_RANK_DESC_BYTES / (int)sizeof(RankSlot<P>));
}
template <int P>
struct RankSlots {
  RankSlot<P> s[rank_chunk<P>()];
};
struct RankThr {
  double t[PS_RANK_MAX_THR];
};

// one count plane of a pair of cells (the tail cell alone: e1 is false there)
__device__ inline void rank_count(uint32_t* __restrict__ plane, int64_t i, bool pair, bool e0, bool e1, uint32_t wi) {
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
// N*N alone).  Every thread of a block makes the same number of trips, so the ballots see whole waves.  Every loop
// over the plans has the constant trip count P and is unrolled: a0, a1 and the counters are registers.
template <int P>
__global__ void __launch_bounds__(PS_RANK_THREADS)
    k_rank_add(RankSlots<P> desc, double* __restrict__ mean, double* __restrict__ m2, uint32_t* __restrict__ cnt,
               uint32_t* __restrict__ row, int64_t ncell, int64_t pitch, int nslot, int nthr, RankThr thr, double w,
               double Wn, uint32_t wi) {
  __shared__ uint32_t part[PS_RANK_THREADS / 64][PS_RANK_MAX_THR * P];
  const RankSlot<P> sd = desc.s[blockIdx.y];
  double* ms = mean + (int64_t)sd.slot * P * pitch;
  double* qs = m2 + (int64_t)sd.slot * P * pitch;
  uint32_t* cs = cnt + (int64_t)sd.slot * (P + nthr * (P + 2)) * pitch;
  const int64_t npair = ncell >> 1;
  const int64_t nitem = npair + (ncell & 1);
  uint32_t na[PS_RANK_MAX_THR][P];
#pragma unroll
  for (int k = 0; k < PS_RANK_MAX_THR; ++k) {
#pragma unroll
    for (int j = 0; j < P; ++j) na[k][j] = 0u;
  }
  for (int64_t base = blockIdx.x * (int64_t)blockDim.x; base < nitem; base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t it = base + threadIdx.x;
    const bool pair = it < npair, live = it < nitem;
    const int64_t i = pair ? 2 * it : ncell - 1;
    double a0[P], a1[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
      a0[j] = 0.0, a1[j] = 0.0;
      if (pair) {
        const double2 r = *reinterpret_cast<const double2*>(sd.a[j] + i);
        a0[j] = r.x, a1[j] = r.y;
      } else if (live) {
        a0[j] = sd.a[j][i];
      }
    }
    if (live) {
      double mx0 = a0[0], mx1 = a1[0];
#pragma unroll
      for (int j = 1; j < P; ++j) {
        mx0 = a0[j] > mx0 ? a0[j] : mx0;
        mx1 = a1[j] > mx1 ? a1[j] : mx1;
      }
      int n0 = 0, n1 = 0;   // the plans that hold the maximum
#pragma unroll
      for (int j = 0; j < P; ++j) {
        n0 += a0[j] == mx0 ? 1 : 0;
        n1 += a1[j] == mx1 ? 1 : 0;
      }
#pragma unroll
      for (int j = 0; j < P; ++j) {
        // the regret of plan j; the tail's second cell: 0 against 0, nothing
        const double r0 = __dsub_rn(mx0, a0[j]), r1 = __dsub_rn(mx1, a1[j]);
        double* mj = ms + (int64_t)j * pitch;
        double* qj = qs + (int64_t)j * pitch;
        // a pair at regret 0 whose means are 0 changes nothing: the check below reads the means only
        double2 m, q;
        if (pair) {
          m = *reinterpret_cast<const double2*>(mj + i);
        } else {
          m = make_double2(mj[i], 0.0);
        }
        if (r0 != m.x || r1 != m.y) {
          if (pair) {
            q = *reinterpret_cast<const double2*>(qj + i);
          } else {
            q = make_double2(qj[i], 0.0);
          }
          sum_update(r0, w, Wn, m.x, q.x);
          sum_update(r1, w, Wn, m.y, q.y);
          if (pair) {
            *reinterpret_cast<double2*>(mj + i) = m;
            *reinterpret_cast<double2*>(qj + i) = q;
          } else {
            mj[i] = m.x;
            qj[i] = q.x;
          }
        }
        rank_count(cs + (int64_t)j * pitch, i, pair, n0 == 1 && a0[j] == mx0, n1 == 1 && a1[j] == mx1, wi);
      }
      for (int k = 0; k < nthr; ++k) {
        const double t = thr.t[k];
        int c0 = 0, c1 = 0;   // the plans that reach t
#pragma unroll
        for (int j = 0; j < P; ++j) {
          c0 += a0[j] >= t ? 1 : 0;
          c1 += a1[j] >= t ? 1 : 0;
        }
        if (c0 | c1) {
          uint32_t* ck = cs + (int64_t)(P + k * (P + 2)) * pitch;
#pragma unroll
          for (int j = 0; j < P; ++j)
            rank_count(ck + (int64_t)j * pitch, i, pair, c0 == 1 && a0[j] >= t, c1 == 1 && a1[j] >= t, wi);
          rank_count(ck + (int64_t)P * pitch, i, pair, c0 >= 1, c1 >= 1, wi);
          rank_count(ck + (int64_t)(P + 1) * pitch, i, pair, c0 == P, c1 == P, wi);
        }
      }
    }
    // the cells each plan covers: a lane without cells holds zeros, below every threshold
#pragma unroll
    for (int k = 0; k < PS_RANK_MAX_THR; ++k) {
      if (k < nthr) {
        const double t = thr.t[k];
#pragma unroll
        for (int j = 0; j < P; ++j)
          na[k][j] += (uint32_t)(__popcll(__ballot(a0[j] >= t)) + __popcll(__ballot(a1[j] >= t)));
      }
    }
  }
  if (nthr == 0) return;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < PS_RANK_MAX_THR; ++k) {
#pragma unroll
      for (int j = 0; j < P; ++j) part[threadIdx.x >> 6][k * P + j] = na[k][j];
    }
  }
  __syncthreads();
  if (threadIdx.x < PS_RANK_MAX_THR * P) {
    const int k = threadIdx.x / P, j = threadIdx.x % P;
    if (k < nthr) {
      uint32_t c = 0;
      for (int v = 0; v < PS_RANK_THREADS / 64; ++v) c += part[v][threadIdx.x];
      if (c) atomicAdd(row + ((int64_t)j * nthr + k) * nslot + sd.slot, c);
    }
  }
}

// Chan, Golub & LeVeque on every mean / M2 pair, with the expressions of k_summary_merge; the counts add
__global__ void k_rank_merge(double* __restrict__ ma, double* __restrict__ qa, uint32_t* __restrict__ ca,
                             const double* __restrict__ mb, const double* __restrict__ qb,
                             const uint32_t* __restrict__ cb, int64_t nval, int64_t ncnt, double Wa, double Wb) {
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

struct ps_rank {
  int device = 0, N = 0, nplan = 0, nslot = 0, nthr = 0;
  std::vector<double> thr;
  int64_t ncell = 0, pitch = 0;
  double* mean = nullptr;        // [slot][plan][pitch]
  double* m2 = nullptr;          // [slot][plan][pitch]
  uint32_t* cnt = nullptr;       // [slot][P + nthr (P + 2)][pitch]
  uint32_t* rows = nullptr;      // [rows_cap][plan][k][slot]; null without thresholds
  int64_t rows_cap = 0;
  uint64_t W = 0;
  int64_t members = 0;
  std::vector<uint32_t> weights;   // per member, in row order
  hipStream_t stream = nullptr;    // every operation of the handle
  PsLastOp last;                   // the last operation
  PsProf prof;                     // channel 0: the adds
};

static int rank_planes(const ps_rank* h) { return h->nplan + h->nthr * (h->nplan + 2); }
static int64_t rank_row_len(const ps_rank* h) { return (int64_t)h->nplan * h->nthr * h->nslot; }
static size_t rank_val_bytes(const ps_rank* h) {
  return (size_t)h->nslot * h->nplan * h->pitch * sizeof(double);
}
static size_t rank_cnt_bytes(const ps_rank* h) {
  return (size_t)h->nslot * rank_planes(h) * h->pitch * sizeof(uint32_t);
}

// room for `need` member rows: a doubling copies the rows so far on the handle's stream and synchronises once
// before the old block is freed
static int rank_reserve_rows(ps_rank* h, int64_t need) {
  if (h->nthr == 0 || need <= h->rows_cap) return PS_OK;
  int64_t cap = std::max<int64_t>(h->rows_cap, PS_RANK_ROWS0);
  while (cap < need) cap *= 2;
  const size_t row_b = (size_t)rank_row_len(h) * sizeof(uint32_t);
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
      return ps_fail(PS_ERR_HIP, "rank: growing the member rows: %s", hipGetErrorString(e));
    }
    PS_HIP(hipFree(h->rows));
  }
  h->rows = p;
  h->rows_cap = cap;
  return PS_OK;
}

extern "C" void ps_rank_destroy(ps_rank* h) {
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

extern "C" int ps_rank_reset(ps_rank* h) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "rank_reset: null handle");
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(h->last.wait(h->stream));
  PS_HIP(hipMemsetAsync(h->mean, 0, rank_val_bytes(h), h->stream));
  PS_HIP(hipMemsetAsync(h->m2, 0, rank_val_bytes(h), h->stream));
  PS_HIP(hipMemsetAsync(h->cnt, 0, rank_cnt_bytes(h), h->stream));
  PS_TRY(h->last.mark(h->stream));
  h->W = 0;
  h->members = 0;
  h->weights.clear();
  return PS_OK;
}

extern "C" int ps_rank_create(int device, int N, int nplan, int nslot, int nthr, const double* thr, ps_rank** out) {
  if (!out || N < 1 || nslot < 1 || nthr < 0 || nthr > PS_RANK_MAX_THR || (nthr > 0 && !thr))
    return ps_fail(PS_ERR_BAD_ARG, "rank_create: N %d, %d slots, %d thresholds (0..%d)", N, nslot, nthr,
                   PS_RANK_MAX_THR);
  *out = nullptr;
  if (nplan < PS_RANK_MIN_PLANS || nplan > PS_RANK_MAX_PLANS)
    return ps_fail(PS_ERR_BAD_ARG, "rank_create: %d plans; %d..%d are ranked", nplan, PS_RANK_MIN_PLANS,
                   PS_RANK_MAX_PLANS);
  for (int k = 0; k < nthr; ++k) {
    if (!(thr[k] > 0.0) || !isfinite(thr[k]))
      return ps_fail(PS_ERR_BAD_ARG, "rank_create: threshold %d = %g is not finite and > 0", k, thr[k]);
    if (k > 0 && !(thr[k] > thr[k - 1]))
      return ps_fail(PS_ERR_BAD_ARG, "rank_create: thresholds not strictly increasing at %d", k);
  }
  PS_TRY(ps_use_device(device));
  const int64_t ncell = (int64_t)N * N;
  const int64_t pitch = (ncell + 63) / 64 * 64;
  // everything, checked before anything is allocated: the moments, the count planes, the first member rows
  const double planes = (double)nplan + (double)nthr * (nplan + 2);
  const double per_cell = 16.0 * nplan + 4.0 * planes;
  const double need = (double)nslot * pitch * per_cell + (double)nplan * nthr * nslot * PS_RANK_ROWS0 * 4.0;
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > (double)free_b)
    return ps_fail(PS_ERR_OOM, "rank_create: %d slots x %lld cells x %g B (%d plans) = %.3g GB, %.3g GB free", nslot,
                   (long long)pitch, per_cell, nplan, need * 1e-9, (double)free_b * 1e-9);
  ps_rank* h = new ps_rank();
  h->device = device;
  h->N = N;
  h->nplan = nplan;
  h->nslot = nslot;
  h->nthr = nthr;
  h->thr.assign(thr, thr + nthr);
  h->ncell = ncell;
  h->pitch = pitch;
  auto fail = [&](int rc) {
    ps_rank_destroy(h);
    return rc;
  };
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = h->last.create();
  if (e == hipSuccess) e = hipMalloc((void**)&h->mean, rank_val_bytes(h));
  if (e == hipSuccess) e = hipMalloc((void**)&h->m2, rank_val_bytes(h));
  if (e == hipSuccess) e = hipMalloc((void**)&h->cnt, rank_cnt_bytes(h));
  if (e != hipSuccess)
    return fail(ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "rank_create: %s", hipGetErrorString(e)));
  int rc = rank_reserve_rows(h, PS_RANK_ROWS0);
  if (rc == PS_OK) rc = ps_rank_reset(h);
  if (rc != PS_OK) return fail(rc);
  *out = h;
  return PS_OK;
}

// the launches of one add over the handle's slots, a chunk of descriptors per launch
template <int P>
static int rank_launch(ps_rank* h, const PsProjectView* v, uint32_t* row, const RankThr& thr, uint32_t weight, double Wn,
                       const char* who) {
  constexpr int chunk = rank_chunk<P>();
  const int64_t nitem = h->ncell / 2 + (h->ncell & 1);
  const int bx = (int)std::min<int64_t>((nitem + PS_RANK_THREADS - 1) / PS_RANK_THREADS, PS_RANK_MAX_BLOCKS);
  for (int c0 = 0; c0 < h->nslot; c0 += chunk) {
    const int n = std::min(chunk, h->nslot - c0);
    RankSlots<P> desc;
    for (int i = 0; i < chunk; ++i) {
      const int e = c0 + i;
      for (int j = 0; j < P; ++j) desc.s[i].a[j] = i < n ? v[j].Y + (int64_t)e * v[j].pitch : nullptr;
      desc.s[i].slot = i < n ? e : 0;
    }
    hipLaunchKernelGGL(k_rank_add<P>, dim3(bx, n), dim3(PS_RANK_THREADS), 0, h->stream, desc, h->mean, h->m2, h->cnt, row,
                       h->ncell, h->pitch, h->nslot, h->nthr, thr, (double)weight, Wn, weight);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ps_fail(PS_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(e));
  }
  return PS_OK;
}

// one member whose values are the current fields of nplan projections or nplan release plans (who: the entry point)
static int rank_add_fields(ps_rank* h, void* const* plans, int nplan, const PsFieldsOps& src, const char* who,
                           uint32_t weight) {
  if (!h || !plans) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  if (nplan < PS_RANK_MIN_PLANS || nplan > PS_RANK_MAX_PLANS || nplan != h->nplan)
    return ps_fail(PS_ERR_BAD_ARG, "%s: %d plans given, the handle ranks %d (%d..%d)", who, nplan, h->nplan,
                   PS_RANK_MIN_PLANS, PS_RANK_MAX_PLANS);
  for (int j = 0; j < nplan; ++j) {
    if (!plans[j]) return ps_fail(PS_ERR_BAD_ARG, "%s: %s %d is null", who, src.what, j);
    for (int i = 0; i < j; ++i)
      if (plans[i] == plans[j])
        return ps_fail(PS_ERR_BAD_ARG, "%s: %s %d and %d are the same handle", who, src.what, i, j);
  }
  if (weight < 1) return ps_fail(PS_ERR_BAD_ARG, "%s: weight must be >= 1", who);
  if (h->W + weight > 0xffffffffull)
    return ps_fail(PS_ERR_BAD_ARG, "%s: total weight %llu would overflow the uint32 counts", who,
                   (unsigned long long)(h->W + weight));
  PsProjectView v[PS_RANK_MAX_PLANS];
  for (int j = 0; j < nplan; ++j) {
    PS_TRY(src.view(plans[j], &v[j]));
    if (v[j].nout != h->nslot)
      return ps_fail(PS_ERR_BAD_ARG, "%s: %s %d has %d outputs, the handle %d slots", who, src.what, j, v[j].nout,
                     h->nslot);
    if (v[j].device != h->device)
      return ps_fail(PS_ERR_BAD_ARG, "%s: %s %d on device %d, handle on device %d", who, src.what, j, v[j].device,
                     h->device);
    if (v[j].N != h->N)
      return ps_fail(PS_ERR_BAD_ARG, "%s: %s %d domain %d, handle domain %d", who, src.what, j, v[j].N, h->N);
  }
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(rank_reserve_rows(h, h->members + 1));
  hipStream_t stream = h->stream;
  for (int j = 0; j < nplan; ++j) PS_TRY(src.wait(plans[j], stream));
  PS_TRY(h->last.wait(stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(h->prof.begin(0, stream, &e1));
  RankThr thr;
  for (int k = 0; k < PS_RANK_MAX_THR; ++k) thr.t[k] = k < h->nthr ? h->thr[(size_t)k] : 0.0;
  uint32_t* row = nullptr;
  if (h->nthr) {   // the member's row: integer sums over the blocks, from zero
    row = h->rows + h->members * rank_row_len(h);
    hipError_t e = hipMemsetAsync(row, 0, (size_t)rank_row_len(h) * sizeof(uint32_t), stream);
    if (e != hipSuccess) return ps_fail(PS_ERR_HIP, "%s: clearing the member's row: %s", who, hipGetErrorString(e));
  }
  const double Wn = (double)(h->W + weight);
  int rc = PS_OK;
  switch (nplan) {
    case 2: rc = rank_launch<2>(h, v, row, thr, weight, Wn, who); break;
    case 3: rc = rank_launch<3>(h, v, row, thr, weight, Wn, who); break;
    case 4: rc = rank_launch<4>(h, v, row, thr, weight, Wn, who); break;
    case 5: rc = rank_launch<5>(h, v, row, thr, weight, Wn, who); break;
    case 6: rc = rank_launch<6>(h, v, row, thr, weight, Wn, who); break;
    case 7: rc = rank_launch<7>(h, v, row, thr, weight, Wn, who); break;
    default: rc = rank_launch<8>(h, v, row, thr, weight, Wn, who); break;
  }
  PS_TRY(rc);
  PS_TRY(h->prof.end(stream, e1));
  PS_TRY(h->last.mark(stream));
  h->W += weight;
  h->members += 1;
  h->weights.push_back(weight);
  // the next apply of any plan overwrites its fields only after this read
  for (int j = 0; j < nplan; ++j) PS_TRY(src.mark(plans[j], stream));
  return PS_OK;
}

extern "C" int ps_rank_add_sites(ps_rank* h, ps_sites* const* plans, int nplan, uint32_t weight) {
  return rank_add_fields(h, (void* const*)plans, nplan, ps_sites_fields(), "rank_add_sites", weight);
}

extern "C" int ps_rank_add_project(ps_rank* h, ps_project* const* plans, int nplan, uint32_t weight) {
  return rank_add_fields(h, (void* const*)plans, nplan, ps_project_fields(), "rank_add_project", weight);
}

extern "C" int ps_rank_merge(ps_rank* dst, ps_rank* src) {
  if (!dst || !src || dst == src) return ps_fail(PS_ERR_BAD_ARG, "rank_merge: bad arguments");
  if (dst->device != src->device || dst->N != src->N || dst->nplan != src->nplan || dst->nslot != src->nslot ||
      dst->thr != src->thr)
    return ps_fail(PS_ERR_BAD_ARG, "rank_merge: handles differ in device, domain, plans, slots or thresholds");
  if (dst->W + src->W > 0xffffffffull) return ps_fail(PS_ERR_BAD_ARG, "rank_merge: total weight would overflow");
  if (src->members == 0) return PS_OK;
  PS_HIP(hipSetDevice(dst->device));
  PS_TRY(rank_reserve_rows(dst, dst->members + src->members));
  PS_TRY(dst->last.wait(dst->stream));
  PS_TRY(src->last.wait(dst->stream));
  if (dst->W == 0) {   // a copy: the merged handle is src bit for bit
    PS_HIP(hipMemcpyAsync(dst->mean, src->mean, rank_val_bytes(dst), hipMemcpyDeviceToDevice, dst->stream));
    PS_HIP(hipMemcpyAsync(dst->m2, src->m2, rank_val_bytes(dst), hipMemcpyDeviceToDevice, dst->stream));
    PS_HIP(hipMemcpyAsync(dst->cnt, src->cnt, rank_cnt_bytes(dst), hipMemcpyDeviceToDevice, dst->stream));
  } else {
    const int64_t ncell = (int64_t)dst->nslot * dst->pitch;
    hipLaunchKernelGGL(k_rank_merge, dim3(2048), dim3(256), 0, dst->stream, dst->mean, dst->m2, dst->cnt, src->mean,
                       src->m2, src->cnt, ncell * dst->nplan, ncell * rank_planes(dst), (double)dst->W, (double)src->W);
    PS_HIP(hipGetLastError());
  }
  if (dst->nthr) {
    const int64_t len = rank_row_len(dst);
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

extern "C" int ps_rank_info(ps_rank* h, double* total_weight, int64_t* members) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "rank_info: null handle");
  if (total_weight) *total_weight = (double)h->W;
  if (members) *members = h->members;
  return PS_OK;
}

extern "C" int ps_rank_fetch_counts(ps_rank* h, int slot, int which, uint32_t* out) {
  if (!h || !out) return ps_fail(PS_ERR_BAD_ARG, "rank_fetch_counts: bad arguments");
  if (slot < 0 || slot >= h->nslot) return ps_fail(PS_ERR_BAD_ARG, "rank_fetch_counts: slot %d of %d", slot, h->nslot);
  if (which < 0 || which >= rank_planes(h))
    return ps_fail(PS_ERR_BAD_ARG,
                   "rank_fetch_counts: plane %d (j best_j, P + k (P + 2) + j sole_kj, then any_k, all_k; %d planes)", which,
                   rank_planes(h));
  if (h->W == 0) return ps_fail(PS_ERR_STATE, "rank_fetch_counts: nothing accumulated (W = 0)");
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(h->last.wait(h->stream));
  const uint32_t* src = h->cnt + ((int64_t)slot * rank_planes(h) + which) * h->pitch;
  PS_HIP(hipMemcpyAsync(out, src, (size_t)h->ncell * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  PS_HIP(hipStreamSynchronize(h->stream));
  return PS_OK;
}

extern "C" int ps_rank_fetch(ps_rank* h, int slot, int plan, int what, double* out) {
  if (!h || !out) return ps_fail(PS_ERR_BAD_ARG, "rank_fetch: bad arguments");
  if (slot < 0 || slot >= h->nslot) return ps_fail(PS_ERR_BAD_ARG, "rank_fetch: slot %d of %d", slot, h->nslot);
  if (plan < 0 || plan >= h->nplan) return ps_fail(PS_ERR_BAD_ARG, "rank_fetch: plan %d of %d", plan, h->nplan);
  if (what < 0 || what > 2)
    return ps_fail(PS_ERR_BAD_ARG, "rank_fetch: quantity %d (0 regret mean, 1 regret variance, 2 P(best))", what);
  if (h->W == 0) return ps_fail(PS_ERR_STATE, "rank_fetch: nothing accumulated (W = 0)");
  const double W = (double)h->W;
  const size_t n = (size_t)h->ncell;
  if (what == 2) {
    std::vector<uint32_t> c(n);
    PS_TRY(ps_rank_fetch_counts(h, slot, plan, c.data()));
    for (size_t i = 0; i < n; ++i) out[i] = (double)c[i] / W;
    return PS_OK;
  }
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(h->last.wait(h->stream));
  const double* src = (what == 0 ? h->mean : h->m2) + ((int64_t)slot * h->nplan + plan) * h->pitch;
  PS_HIP(hipMemcpyAsync(out, src, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  PS_HIP(hipStreamSynchronize(h->stream));
  if (what == 1)
    for (size_t i = 0; i < n; ++i) out[i] /= W;
  return PS_OK;
}

extern "C" int ps_rank_fetch_coverage(ps_rank* h, int64_t first, int64_t count, uint32_t* cells, uint32_t* weights) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "rank_fetch_coverage: null handle");
  if (first < 0 || count < 0 || first + count > h->members)
    return ps_fail(PS_ERR_BAD_ARG, "rank_fetch_coverage: members %lld .. %lld of %lld", (long long)first,
                   (long long)(first + count), (long long)h->members);
  if (weights)
    for (int64_t m = 0; m < count; ++m) weights[m] = h->weights[(size_t)(first + m)];
  if (!cells || count == 0 || h->nthr == 0) return PS_OK;
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(h->last.wait(h->stream));
  const int64_t len = rank_row_len(h);
  PS_HIP(hipMemcpyAsync(cells, h->rows + first * len, (size_t)(count * len) * sizeof(uint32_t), hipMemcpyDeviceToHost,
                        h->stream));
  PS_HIP(hipStreamSynchronize(h->stream));
  return PS_OK;
}

extern "C" int ps_rank_prof(ps_rank* h, int enable, double* total_ms, int64_t* launches) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "rank_prof: null handle");
  PS_HIP(hipSetDevice(h->device));
  h->prof.set(enable);
  if (total_ms || launches) PS_TRY(h->prof.totals(0, total_ms, launches));
  return PS_OK;
}
