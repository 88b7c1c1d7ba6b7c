// Monte Carlo error of the posterior maps (include/parasitoid_hip.h, ps_mcerr_*): batch means of one sequence
// of members -- a chain, or half of one -- kept on the device.  The sequence is cut into batches of exactly b
// rows of weight; an add of any weight is split by the library at the batch boundaries.  Layout (pitch = N*N
// rounded up to 64 cells, as ps_summary.hip):
//   bmean[slot][pitch], bM2[slot][pitch]   fp64, the open batch: the step of ps_summary.hip (sum_update)
//   gmean[slot][pitch], gM2[slot][pitch]   fp64, Welford over the closed batches' means, weight 1 each
//   wM2[slot][pitch]                       fp64, the sum of the closed batches' own M2
//   bcnt[slot][k][pitch]                   uint32, the open batch's weight with value >= t_k
//   s1[slot][k][pitch]                     uint32, the sum of the closed batches' counts
//   s2[slot][k][pitch]                     uint64, the sum of their squares
// An add reads 8 B of record and reads + writes 16 B of bmean, 16 B of bM2 and 8 B per threshold of every cell
// of every slot, less where a pair of cells is unchanged; a close reads the five fp64 planes and the three
// count planes once and stores only where something changes.  One thread owns a pair of cells throughout, so
// every cell has a single writer: no atomics, and the counts are exact integers (total weight <= 2^32 - 1, so
// s2 <= n b < 2^64).
#include <math.h>

#include <algorithm>
#include <vector>

#include "ps_common.h"

#define PS_MCE_MAX_THR 4
#define PS_MCE_CHUNK 32          // slots per launch: 32 descriptors = 1.3 kB of kernel arguments
#define PS_MCE_THREADS 256
#define PS_MCE_MAX_BLOCKS 4096   // per slot, as ps_summary.hip; more pairs than 4096 x 256 take the grid stride
#define PS_MCE_MAX_SEQ 16        // sequences of one R-hat

namespace {

struct MceSlot {
  const double* rec;
  const ps_day_stats* stats;   // nullptr: no delta
  double stat_scale, post_scale;
  int slot;
};
struct MceSlots {
  MceSlot s[PS_MCE_CHUNK];
};
struct MceThr {
  double t[PS_MCE_MAX_THR];
};

// blockIdx.y = slot of the chunk; a thread owns a pair of cells (the tail cell of an odd N*N alone).  w: the
// piece's weight, Wn: the open batch's weight with it.
__global__ void __launch_bounds__(PS_MCE_THREADS)
    k_mcerr_add(MceSlots desc, double* __restrict__ bmean, double* __restrict__ bm2, uint32_t* __restrict__ bcnt,
                int64_t ncell, int64_t pitch, int nthr, MceThr thr, double negval, double w, double Wn, uint32_t wi) {
  const MceSlot sd = desc.s[blockIdx.y];
  const double delta = sd.stats ? sd.stats->delta : 0.0;
  const double* __restrict__ rec = sd.rec;
  double* ms = bmean + (int64_t)sd.slot * pitch;
  double* qs = bm2 + (int64_t)sd.slot * pitch;
  uint32_t* cs = bcnt + (int64_t)sd.slot * nthr * pitch;
  const int64_t npair = ncell >> 1;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j <= npair; j += (int64_t)gridDim.x * blockDim.x) {
    if (j < npair) {
      const double2 r = *reinterpret_cast<const double2*>(rec + 2 * j);
      double2 m = *reinterpret_cast<const double2*>(ms + 2 * j);
      double2 q = *reinterpret_cast<const double2*>(qs + 2 * j);
      const double v0 = ps_record_value(r.x, sd.stat_scale, sd.post_scale, delta, negval);
      const double v1 = ps_record_value(r.y, sd.stat_scale, sd.post_scale, delta, negval);
      const bool c0 = sum_update(v0, w, Wn, m.x, q.x);
      const bool c1 = sum_update(v1, w, Wn, m.y, q.y);
      if (c0 || c1) {
        *reinterpret_cast<double2*>(ms + 2 * j) = m;
        *reinterpret_cast<double2*>(qs + 2 * j) = q;
      }
      for (int k = 0; k < nthr; ++k) {
        const bool e0 = v0 >= thr.t[k], e1 = v1 >= thr.t[k];
        if (e0 || e1) {
          uint2* p = reinterpret_cast<uint2*>(cs + (int64_t)k * pitch + 2 * j);
          uint2 c = *p;
          c.x += e0 ? wi : 0u;
          c.y += e1 ? wi : 0u;
          *p = c;
        }
      }
    } else if (ncell & 1) {
      const int64_t i = ncell - 1;
      const double v = ps_record_value(rec[i], sd.stat_scale, sd.post_scale, delta, negval);
      double m = ms[i], q = qs[i];
      if (sum_update(v, w, Wn, m, q)) {
        ms[i] = m;
        qs[i] = q;
      }
      for (int k = 0; k < nthr; ++k)
        if (v >= thr.t[k]) cs[(int64_t)k * pitch + i] += wi;
    }
  }
}

// The open batch becomes closed batch number Bn: its mean one Welford step of (gmean, gM2) with weight 1, its M2
// onto wM2, its counts onto s1 and their squares onto s2; then the batch planes are zero again.  Pairs of cells
// over all slots (nval = nslot * pitch, a multiple of 64) and over all count planes (ncnt = nval * nthr).
__global__ void __launch_bounds__(PS_MCE_THREADS)
    k_mcerr_close(double* __restrict__ bmean, double* __restrict__ bm2, double* __restrict__ gmean,
                  double* __restrict__ gm2, double* __restrict__ wm2, uint32_t* __restrict__ bcnt,
                  uint32_t* __restrict__ s1, uint64_t* __restrict__ s2, int64_t nval, int64_t ncnt, double Bn) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t first = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (int64_t j = first; 2 * j < nval; j += stride) {
    const double2 m = *reinterpret_cast<const double2*>(bmean + 2 * j);
    const double2 q = *reinterpret_cast<const double2*>(bm2 + 2 * j);
    double2 g = *reinterpret_cast<const double2*>(gmean + 2 * j);
    if (m.x != g.x || m.y != g.y) {   // sum_update changes nothing where the batch mean equals gmean
      double2 h = *reinterpret_cast<const double2*>(gm2 + 2 * j);
      sum_update(m.x, 1.0, Bn, g.x, h.x);
      sum_update(m.y, 1.0, Bn, g.y, h.y);
      *reinterpret_cast<double2*>(gmean + 2 * j) = g;
      *reinterpret_cast<double2*>(gm2 + 2 * j) = h;
    }
    if (q.x != 0.0 || q.y != 0.0) {
      double2 s = *reinterpret_cast<const double2*>(wm2 + 2 * j);
      s.x += q.x;
      s.y += q.y;
      *reinterpret_cast<double2*>(wm2 + 2 * j) = s;
      *reinterpret_cast<double2*>(bm2 + 2 * j) = make_double2(0.0, 0.0);
    }
    if (m.x != 0.0 || m.y != 0.0) *reinterpret_cast<double2*>(bmean + 2 * j) = make_double2(0.0, 0.0);
  }
  for (int64_t j = first; 2 * j < ncnt; j += stride) {
    const uint2 c = *reinterpret_cast<const uint2*>(bcnt + 2 * j);
    if (c.x | c.y) {
      uint2 a = *reinterpret_cast<const uint2*>(s1 + 2 * j);
      ulonglong2 b = *reinterpret_cast<const ulonglong2*>(s2 + 2 * j);
      a.x += c.x;
      a.y += c.y;
      b.x += (uint64_t)c.x * c.x;
      b.y += (uint64_t)c.y * c.y;
      *reinterpret_cast<uint2*>(s1 + 2 * j) = a;
      *reinterpret_cast<ulonglong2*>(s2 + 2 * j) = b;
      *reinterpret_cast<uint2*>(bcnt + 2 * j) = make_uint2(0u, 0u);
    }
  }
}

// Chan, Golub & LeVeque on (gmean, gM2) with the batch counts, the expressions of k_summary_merge; wM2, s1 and
// s2 add
__global__ void k_mcerr_merge(double* __restrict__ ma, double* __restrict__ qa, double* __restrict__ wa,
                              uint32_t* __restrict__ s1a, uint64_t* __restrict__ s2a, const double* __restrict__ mb,
                              const double* __restrict__ qb, const double* __restrict__ wb,
                              const uint32_t* __restrict__ s1b, const uint64_t* __restrict__ s2b, int64_t nval,
                              int64_t ncnt, double Ba, double Bb) {
  const double B = Ba + Bb;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nval; i += stride) {
    const double d = mb[i] - ma[i];
    ma[i] = ma[i] + d * (Bb / B);
    qa[i] = qa[i] + qb[i] + d * d * (Ba * Bb / B);
    wa[i] = wa[i] + wb[i];
  }
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < ncnt; i += stride) {
    s1a[i] += s1b[i];
    s2a[i] += s2b[i];
  }
}

struct MceSeqs {
  const double* gmean[PS_MCE_MAX_SEQ];
  const double* gm2[PS_MCE_MAX_SEQ];
  const double* wm2[PS_MCE_MAX_SEQ];
  double n[PS_MCE_MAX_SEQ];   // used weight b B_j
};

// split R-hat of one slot over nh sequences, taken in argument order; 0 where the mean within-sequence
// variance is 0 (a cell that is constant in every sequence)
__global__ void __launch_bounds__(PS_MCE_THREADS)
    k_mcerr_rhat(MceSeqs seq, int nh, double b, double nbar, int64_t ncell, double* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < ncell; i += stride) {
    double W = 0.0, msum = 0.0;
    for (int j = 0; j < nh; ++j) {
      const double s2 = (seq.wm2[j][i] + b * seq.gm2[j][i]) / (seq.n[j] - 1.0);
      W += s2;
      msum += seq.gmean[j][i];
    }
    W /= (double)nh;
    const double mbar = msum / (double)nh;
    double Bv = 0.0;
    for (int j = 0; j < nh; ++j) {
      const double d = seq.gmean[j][i] - mbar;
      Bv += d * d;
    }
    Bv /= (double)(nh - 1);
    out[i] = W == 0.0 ? 0.0 : sqrt(((nbar - 1.0) / nbar * W + Bv) / W);
  }
}

}  // namespace

struct ps_mcerr {
  int device = 0, N = 0, nslot = 0, nthr = 0;
  std::vector<double> thr;
  int64_t ncell = 0, pitch = 0;
  uint32_t b = 0;                 // batch weight
  double* val = nullptr;          // five fp64 planes of [slot][pitch]: bmean, bM2, gmean, gM2, wM2
  uint32_t* bcnt = nullptr;       // [slot][k][pitch]
  uint32_t* s1 = nullptr;
  uint64_t* s2 = nullptr;
  double* scratch = nullptr;      // [pitch], the R-hat plane; allocated at the first ps_mcerr_rhat
  uint64_t B = 0;                 // closed batches
  uint64_t open = 0;              // weight in the open batch, < b
  uint64_t discarded = 0;
  uint64_t W = 0;                 // every weight added: b B + open + discarded
  int64_t members = 0;
  hipStream_t stream = nullptr;   // reset / finish / merge / fetch / rhat
  PsLastOp last;                  // the last operation, on whatever stream it ran
  PsProf prof;                    // channel 0: the adds, 1: the batch closes
};

static size_t mce_plane(const ps_mcerr* h) { return (size_t)h->nslot * h->pitch; }
static double* mce_val(const ps_mcerr* h, int which) { return h->val + (size_t)which * mce_plane(h); }
enum { MCE_BMEAN = 0, MCE_BM2 = 1, MCE_GMEAN = 2, MCE_GM2 = 3, MCE_WM2 = 4 };

extern "C" void ps_mcerr_destroy(ps_mcerr* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  h->last.sync();
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->prof.release();
  for (void* p : {(void*)h->val, (void*)h->bcnt, (void*)h->s1, (void*)h->s2, (void*)h->scratch})
    if (p) (void)hipFree(p);
  h->last.destroy();
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

// the batch planes to zero on `stream`
static int mce_zero_batch(ps_mcerr* h, hipStream_t stream) {
  PS_HIP(hipMemsetAsync(mce_val(h, MCE_BMEAN), 0, 2 * mce_plane(h) * sizeof(double), stream));
  if (h->nthr) PS_HIP(hipMemsetAsync(h->bcnt, 0, mce_plane(h) * h->nthr * sizeof(uint32_t), stream));
  return PS_OK;
}

extern "C" int ps_mcerr_reset(ps_mcerr* h) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "mcerr_reset: null handle");
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(h->last.wait(h->stream));
  PS_HIP(hipMemsetAsync(h->val, 0, 5 * mce_plane(h) * sizeof(double), h->stream));
  if (h->nthr) {
    PS_HIP(hipMemsetAsync(h->bcnt, 0, mce_plane(h) * h->nthr * sizeof(uint32_t), h->stream));
    PS_HIP(hipMemsetAsync(h->s1, 0, mce_plane(h) * h->nthr * sizeof(uint32_t), h->stream));
    PS_HIP(hipMemsetAsync(h->s2, 0, mce_plane(h) * h->nthr * sizeof(uint64_t), h->stream));
  }
  PS_TRY(h->last.mark(h->stream));
  h->B = h->open = h->discarded = h->W = 0;
  h->members = 0;
  return PS_OK;
}

extern "C" int ps_mcerr_create(int device, int N, int nslot, int nthr, const double* thr, uint32_t batch_weight,
                               ps_mcerr** out) {
  if (!out || N < 1 || nslot < 1 || nthr < 0 || nthr > PS_MCE_MAX_THR || (nthr > 0 && !thr))
    return ps_fail(PS_ERR_BAD_ARG, "mcerr_create: N %d, %d slots, %d thresholds (0..%d)", N, nslot, nthr,
                   PS_MCE_MAX_THR);
  *out = nullptr;
  if (batch_weight < 1) return ps_fail(PS_ERR_BAD_ARG, "mcerr_create: batch_weight must be >= 1");
  for (int k = 0; k < nthr; ++k) {
    if (!isfinite(thr[k])) return ps_fail(PS_ERR_BAD_ARG, "mcerr_create: threshold %d = %g is not finite", k, thr[k]);
    if (k > 0 && !(thr[k] > thr[k - 1]))
      return ps_fail(PS_ERR_BAD_ARG, "mcerr_create: thresholds not strictly increasing at %d", k);
  }
  PS_TRY(ps_use_device(device));
  const int64_t ncell = (int64_t)N * N;
  const int64_t pitch = (ncell + 63) / 64 * 64;
  // everything, checked before anything is allocated: five fp64 planes, 16 B of counts per threshold, the R-hat plane
  const double per_cell = 40.0 + 16.0 * nthr;
  const double need = (double)nslot * pitch * per_cell + (double)pitch * 8.0;
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > (double)free_b)
    return ps_fail(PS_ERR_OOM, "mcerr_create: %d slots x %lld cells x %g B = %.3g GB, %.3g GB free", nslot,
                   (long long)pitch, per_cell, need * 1e-9, (double)free_b * 1e-9);
  ps_mcerr* h = new ps_mcerr();
  h->device = device;
  h->N = N;
  h->nslot = nslot;
  h->nthr = nthr;
  h->thr.assign(thr, thr + nthr);
  h->ncell = ncell;
  h->pitch = pitch;
  h->b = batch_weight;
  auto fail = [&](int rc) {
    ps_mcerr_destroy(h);
    return rc;
  };
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = h->last.create();
  if (e == hipSuccess) e = hipMalloc((void**)&h->val, 5 * mce_plane(h) * sizeof(double));
  if (e == hipSuccess && nthr) e = hipMalloc((void**)&h->bcnt, mce_plane(h) * nthr * sizeof(uint32_t));
  if (e == hipSuccess && nthr) e = hipMalloc((void**)&h->s1, mce_plane(h) * nthr * sizeof(uint32_t));
  if (e == hipSuccess && nthr) e = hipMalloc((void**)&h->s2, mce_plane(h) * nthr * sizeof(uint64_t));
  if (e != hipSuccess)
    return fail(ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "mcerr_create: %s", hipGetErrorString(e)));
  int rc = ps_mcerr_reset(h);
  if (rc != PS_OK) return fail(rc);
  *out = h;
  return PS_OK;
}

// a timing pair on `channel` around what `body` enqueues on `stream` (nothing without profiling)
template <typename F>
static int mce_timed(ps_mcerr* h, int channel, hipStream_t stream, F body) {
  hipEvent_t e1 = nullptr;
  PS_TRY(h->prof.begin(channel, stream, &e1));
  PS_TRY(body());
  return h->prof.end(stream, e1);
}

// One member from the slot descriptors d (one per slot), enqueued on `stream`: the weight is split at the batch
// boundaries -- the open batch is filled and closed, then whole batches of b, then the rest -- and every piece is
// one launch of the add kernel on the same source.
static int mce_launch(ps_mcerr* h, const std::vector<PsSrc>& d, hipStream_t stream, double negval, uint32_t weight) {
  PS_TRY(h->last.wait(stream));
  MceThr thr;
  for (int k = 0; k < PS_MCE_MAX_THR; ++k) thr.t[k] = k < h->nthr ? h->thr[(size_t)k] : 0.0;
  const int64_t npair = h->ncell / 2 + 1;
  const int bx = (int)std::min<int64_t>((npair + PS_MCE_THREADS - 1) / PS_MCE_THREADS, PS_MCE_MAX_BLOCKS);
  const int64_t nval = (int64_t)mce_plane(h);
  const int64_t ncnt = nval * h->nthr;
  const int cbx = (int)std::min<int64_t>((std::max(nval, ncnt) / 2 + PS_MCE_THREADS - 1) / PS_MCE_THREADS, 8192);
  uint64_t left = weight;
  int rc = PS_OK;
  while (left > 0 && rc == PS_OK) {
    const uint32_t piece = (uint32_t)std::min<uint64_t>(left, h->b - h->open);
    const double Wn = (double)(h->open + piece);
    rc = mce_timed(h, 0, stream, [&]() {
      for (int c0 = 0; c0 < h->nslot; c0 += PS_MCE_CHUNK) {
        const int n = std::min(PS_MCE_CHUNK, h->nslot - c0);
        MceSlots desc;
        for (int i = 0; i < PS_MCE_CHUNK; ++i)
          desc.s[i] = i < n ? ps_slotted<MceSlot>(d[(size_t)(c0 + i)], c0 + i) : MceSlot{nullptr, nullptr, 0.0, 0.0, 0};
        hipLaunchKernelGGL(k_mcerr_add, dim3(bx, n), dim3(PS_MCE_THREADS), 0, stream, desc, mce_val(h, MCE_BMEAN),
                           mce_val(h, MCE_BM2), h->bcnt, h->ncell, h->pitch, h->nthr, thr, negval, (double)piece, Wn,
                           piece);
        PS_HIP(hipGetLastError());
      }
      return (int)PS_OK;
    });
    if (rc != PS_OK) break;
    h->open += piece;
    h->W += piece;
    left -= piece;
    if (h->open == h->b) {
      rc = mce_timed(h, 1, stream, [&]() {
        hipLaunchKernelGGL(k_mcerr_close, dim3(cbx), dim3(PS_MCE_THREADS), 0, stream, mce_val(h, MCE_BMEAN),
                           mce_val(h, MCE_BM2), mce_val(h, MCE_GMEAN), mce_val(h, MCE_GM2), mce_val(h, MCE_WM2), h->bcnt,
                           h->s1, h->s2, nval, ncnt, (double)(h->B + 1));
        PS_HIP(hipGetLastError());
        return (int)PS_OK;
      });
      if (rc != PS_OK) break;
      h->B += 1;
      h->open = 0;
    }
  }
  PS_TRY(h->last.mark(stream));
  if (rc == PS_OK) h->members += 1;
  return rc;
}

static int mce_check_weight(ps_mcerr* h, const char* who, uint32_t weight) {
  if (weight < 1) return ps_fail(PS_ERR_BAD_ARG, "%s: weight must be >= 1", who);
  if (h->W + weight > 0xffffffffull)
    return ps_fail(PS_ERR_BAD_ARG, "%s: total weight %llu would overflow the uint32 counts", who,
                   (unsigned long long)(h->W + weight));
  return PS_OK;
}

extern "C" int ps_mcerr_add(ps_mcerr* h, ps_solver* s, int nslot, const int32_t* kind, const int32_t* idx,
                            const double* stat_scale, const double* post_scale, const int32_t* use_delta,
                            double negval, uint32_t weight) {
  if (!h || !s || !kind || !idx || !stat_scale || !post_scale || !use_delta)
    return ps_fail(PS_ERR_BAD_ARG, "mcerr_add: bad arguments");
  if (nslot != h->nslot) return ps_fail(PS_ERR_BAD_ARG, "mcerr_add: %d slots given, the handle has %d", nslot, h->nslot);
  PS_TRY(mce_check_weight(h, "mcerr_add", weight));
  PS_HIP(hipSetDevice(h->device));
  // every descriptor first: an add with a bad slot enqueues nothing
  std::vector<PsSrc> d((size_t)nslot);
  hipStream_t stream = nullptr;
  PS_TRY(ps_read_records("mcerr_add", "handle", h->device, h->N, s, nslot, kind, idx, stat_scale, post_scale, use_delta,
                         false, d.data(), &stream));
  return mce_launch(h, d, stream, negval, weight);
}

// one member whose values are the current fields of a projection or a release plan (who: the entry point)
static int mce_add_fields(ps_mcerr* h, void* p, const PsFieldsOps& src, const char* who, uint32_t weight) {
  if (!h || !p) return ps_fail(PS_ERR_BAD_ARG, "%s: bad arguments", who);
  PS_TRY(mce_check_weight(h, who, weight));
  // slot e takes Y_e: no statistics, both scales 1 and negval 0, so the value rule returns Y itself
  std::vector<PsSrc> d((size_t)h->nslot);
  PS_TRY(ps_read_fields(who, "handle", "slots", h->device, h->N, h->nslot, p, src, d.data()));
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(src.wait(p, h->stream));
  PS_TRY(mce_launch(h, d, h->stream, 0.0, weight));
  return src.mark(p, h->stream);   // the next apply overwrites Y only after this read
}

extern "C" int ps_mcerr_add_project(ps_mcerr* h, ps_project* p, uint32_t weight) {
  return mce_add_fields(h, p, ps_project_fields(), "mcerr_add_project", weight);
}

extern "C" int ps_mcerr_add_sites(ps_mcerr* h, ps_sites* p, uint32_t weight) {
  return mce_add_fields(h, p, ps_sites_fields(), "mcerr_add_sites", weight);
}

extern "C" int ps_mcerr_add_catch(ps_mcerr* h, ps_catch* p, uint32_t weight) {
  return mce_add_fields(h, p, ps_catch_fields(), "mcerr_add_catch", weight);
}

extern "C" int ps_mcerr_add_nbhd(ps_mcerr* h, ps_nbhd* p, uint32_t weight) {
  return mce_add_fields(h, p, ps_nbhd_fields(), "mcerr_add_nbhd", weight);
}

extern "C" int ps_mcerr_add_prox(ps_mcerr* h, ps_prox* p, uint32_t weight) {
  return mce_add_fields(h, p, ps_prox_fields(), "mcerr_add_prox", weight);
}

extern "C" int ps_mcerr_finish(ps_mcerr* h) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "mcerr_finish: null handle");
  if (h->open == 0) return PS_OK;
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(h->last.wait(h->stream));
  PS_TRY(mce_zero_batch(h, h->stream));
  PS_TRY(h->last.mark(h->stream));
  h->discarded += h->open;
  h->open = 0;
  return PS_OK;
}

extern "C" int ps_mcerr_merge(ps_mcerr* dst, ps_mcerr* src) {
  if (!dst || !src || dst == src) return ps_fail(PS_ERR_BAD_ARG, "mcerr_merge: bad arguments");
  if (dst->device != src->device || dst->N != src->N || dst->nslot != src->nslot || dst->thr != src->thr)
    return ps_fail(PS_ERR_BAD_ARG, "mcerr_merge: handles differ in device, domain, slots or thresholds");
  if (dst->b != src->b)
    return ps_fail(PS_ERR_BAD_ARG, "mcerr_merge: batch weight %u against %u", (unsigned)dst->b, (unsigned)src->b);
  if (dst->W + src->W > 0xffffffffull) return ps_fail(PS_ERR_BAD_ARG, "mcerr_merge: total weight would overflow");
  if (dst->open || src->open)
    return ps_fail(PS_ERR_STATE, "mcerr_merge: an open batch of weight %llu (finish first)",
                   (unsigned long long)(dst->open ? dst->open : src->open));
  if (src->B > 0) {
    PS_HIP(hipSetDevice(dst->device));
    PS_TRY(dst->last.wait(dst->stream));
    PS_TRY(src->last.wait(dst->stream));
    const size_t nval = mce_plane(dst), ncnt = nval * dst->nthr;
    if (dst->B == 0) {   // a copy: the merged handle is src bit for bit (the batch planes of both are zero)
      PS_HIP(hipMemcpyAsync(dst->val, src->val, 5 * nval * sizeof(double), hipMemcpyDeviceToDevice, dst->stream));
      if (dst->nthr) {
        PS_HIP(hipMemcpyAsync(dst->s1, src->s1, ncnt * sizeof(uint32_t), hipMemcpyDeviceToDevice, dst->stream));
        PS_HIP(hipMemcpyAsync(dst->s2, src->s2, ncnt * sizeof(uint64_t), hipMemcpyDeviceToDevice, dst->stream));
      }
    } else {
      hipLaunchKernelGGL(k_mcerr_merge, dim3(2048), dim3(256), 0, dst->stream, mce_val(dst, MCE_GMEAN),
                         mce_val(dst, MCE_GM2), mce_val(dst, MCE_WM2), dst->s1, dst->s2, mce_val(src, MCE_GMEAN),
                         mce_val(src, MCE_GM2), mce_val(src, MCE_WM2), src->s1, src->s2, (int64_t)nval, (int64_t)ncnt,
                         (double)dst->B, (double)src->B);
      PS_HIP(hipGetLastError());
    }
    PS_TRY(dst->last.mark(dst->stream));
    PS_TRY(src->last.mark(dst->stream));   // src is read until then
  }
  dst->B += src->B;
  dst->W += src->W;
  dst->discarded += src->discarded;
  dst->members += src->members;
  return PS_OK;
}

extern "C" int ps_mcerr_info(ps_mcerr* h, int64_t* batches, int64_t* batch_weight, int64_t* used_weight,
                             int64_t* open_weight, int64_t* discarded_weight, int64_t* members) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "mcerr_info: null handle");
  if (batches) *batches = (int64_t)h->B;
  if (batch_weight) *batch_weight = (int64_t)h->b;
  if (used_weight) *used_weight = (int64_t)(h->B * h->b);
  if (open_weight) *open_weight = (int64_t)h->open;
  if (discarded_weight) *discarded_weight = (int64_t)h->discarded;
  if (members) *members = h->members;
  return PS_OK;
}

static int mce_check_fetch(ps_mcerr* h, const char* who, int slot) {
  if (slot < 0 || slot >= h->nslot) return ps_fail(PS_ERR_BAD_ARG, "%s: slot %d of %d", who, slot, h->nslot);
  return PS_OK;
}

extern "C" int ps_mcerr_fetch(ps_mcerr* h, int slot, int what, double* out) {
  if (!h || !out) return ps_fail(PS_ERR_BAD_ARG, "mcerr_fetch: bad arguments");
  PS_TRY(mce_check_fetch(h, "mcerr_fetch", slot));
  if (what < 0 || what > 2) return ps_fail(PS_ERR_BAD_ARG, "mcerr_fetch: quantity %d (0 gmean, 1 gM2, 2 wM2)", what);
  if (h->B < 2) return ps_fail(PS_ERR_STATE, "mcerr_fetch: %llu closed batches, 2 needed", (unsigned long long)h->B);
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(h->last.wait(h->stream));
  const double* src = mce_val(h, MCE_GMEAN + what) + (int64_t)slot * h->pitch;
  PS_HIP(hipMemcpyAsync(out, src, (size_t)h->ncell * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  PS_HIP(hipStreamSynchronize(h->stream));
  return PS_OK;
}

extern "C" int ps_mcerr_fetch_counts(ps_mcerr* h, int slot, int k, uint32_t* s1, uint64_t* s2) {
  if (!h || (!s1 && !s2)) return ps_fail(PS_ERR_BAD_ARG, "mcerr_fetch_counts: bad arguments");
  PS_TRY(mce_check_fetch(h, "mcerr_fetch_counts", slot));
  if (k < 0 || k >= h->nthr) return ps_fail(PS_ERR_BAD_ARG, "mcerr_fetch_counts: threshold %d of %d", k, h->nthr);
  if (h->B < 2)
    return ps_fail(PS_ERR_STATE, "mcerr_fetch_counts: %llu closed batches, 2 needed", (unsigned long long)h->B);
  PS_HIP(hipSetDevice(h->device));
  PS_TRY(h->last.wait(h->stream));
  const int64_t off = ((int64_t)slot * h->nthr + k) * h->pitch;
  if (s1) PS_HIP(hipMemcpyAsync(s1, h->s1 + off, (size_t)h->ncell * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  if (s2) PS_HIP(hipMemcpyAsync(s2, h->s2 + off, (size_t)h->ncell * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
  PS_HIP(hipStreamSynchronize(h->stream));
  return PS_OK;
}

extern "C" int ps_mcerr_rhat(ps_mcerr* const* handles, int nh, int slot, double* out) {
  if (!handles || !out) return ps_fail(PS_ERR_BAD_ARG, "mcerr_rhat: bad arguments");
  if (nh < 2 || nh > PS_MCE_MAX_SEQ)
    return ps_fail(PS_ERR_BAD_ARG, "mcerr_rhat: %d sequences (2..%d)", nh, PS_MCE_MAX_SEQ);
  for (int j = 0; j < nh; ++j)
    if (!handles[j]) return ps_fail(PS_ERR_BAD_ARG, "mcerr_rhat: sequence %d is null", j);
  ps_mcerr* h0 = handles[0];
  PS_TRY(mce_check_fetch(h0, "mcerr_rhat", slot));
  for (int j = 1; j < nh; ++j) {
    const ps_mcerr* h = handles[j];
    if (h->device != h0->device || h->N != h0->N || h->nslot != h0->nslot || h->b != h0->b)
      return ps_fail(PS_ERR_BAD_ARG, "mcerr_rhat: sequence %d differs in device, domain, slots or batch weight", j);
  }
  for (int j = 0; j < nh; ++j) {
    if (handles[j]->open)
      return ps_fail(PS_ERR_STATE, "mcerr_rhat: sequence %d has an open batch of weight %llu (finish first)", j,
                     (unsigned long long)handles[j]->open);
    if (handles[j]->B < 2)
      return ps_fail(PS_ERR_STATE, "mcerr_rhat: sequence %d has %llu closed batches, 2 needed", j,
                     (unsigned long long)handles[j]->B);
  }
  PS_HIP(hipSetDevice(h0->device));
  if (!h0->scratch) PS_HIP(hipMalloc((void**)&h0->scratch, (size_t)h0->pitch * sizeof(double)));
  MceSeqs seq;
  double nsum = 0.0;
  for (int j = 0; j < PS_MCE_MAX_SEQ; ++j) {
    ps_mcerr* h = handles[j < nh ? j : 0];
    seq.gmean[j] = mce_val(h, MCE_GMEAN) + (int64_t)slot * h->pitch;
    seq.gm2[j] = mce_val(h, MCE_GM2) + (int64_t)slot * h->pitch;
    seq.wm2[j] = mce_val(h, MCE_WM2) + (int64_t)slot * h->pitch;
    seq.n[j] = (double)(h->B * h->b);
    if (j < nh) nsum += seq.n[j];
  }
  hipStream_t stream = h0->stream;
  for (int j = 0; j < nh; ++j) PS_TRY(handles[j]->last.wait(stream));
  const int bx = (int)std::min<int64_t>((h0->ncell + PS_MCE_THREADS - 1) / PS_MCE_THREADS, PS_MCE_MAX_BLOCKS);
  hipLaunchKernelGGL(k_mcerr_rhat, dim3(bx), dim3(PS_MCE_THREADS), 0, stream, seq, nh, (double)h0->b, nsum / (double)nh,
                     h0->ncell, h0->scratch);
  PS_HIP(hipGetLastError());
  PS_HIP(hipMemcpyAsync(out, h0->scratch, (size_t)h0->ncell * sizeof(double), hipMemcpyDeviceToHost, stream));
  for (int j = 0; j < nh; ++j) PS_TRY(handles[j]->last.mark(stream));   // every sequence is read until then
  PS_HIP(hipStreamSynchronize(stream));
  return PS_OK;
}

extern "C" int ps_mcerr_prof(ps_mcerr* h, int enable, double* add_ms, int64_t* add_launches, double* close_ms,
                             int64_t* close_launches) {
  if (!h) return ps_fail(PS_ERR_BAD_ARG, "mcerr_prof: null handle");
  PS_HIP(hipSetDevice(h->device));
  h->prof.set(enable);
  if (add_ms || add_launches) PS_TRY(h->prof.totals(0, add_ms, add_launches));
  if (close_ms || close_launches) PS_TRY(h->prof.totals(1, close_ms, close_launches));
  return PS_OK;
}
