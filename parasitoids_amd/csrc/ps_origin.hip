// Origin maps (include/parasitoid_hip.h, ps_origin_*): given findings -- trap readings in the format of the
// reweighting probes -- the likelihood of every candidate origin cell at once, member by member.  One wind
// station and a homogeneous landscape make the field of a release at cell s the centre release translated
// (ps_sites.hip), the chain is linear in the released number, and a release `lag` days later is a model of its
// own, so under hypothesis h = (amount_h, lag_h) the finding o at cell (r_o, c_o) on day d_o sees
//   v = v_{lag, d_o - lag}(r_o + R - r, c_o + R - c),   mu = (rate_o * amount_h) * v
// with v the value ps_summary_add adds (ps_record_value), 0 outside [0, N) on either axis and 0 before the
// release; l_{m,h}(s) = sum over o of the probe log-likelihood at mu (origin_term, ps_origin_core.h).  Layout
// (pitch = N*N rounded up to 64 cells, as ps_summary.hip):
//   A[h][pitch], S[h][pitch]   fp64: the running maximum and the scaled sum of the members' l (origin_lse_add)
//   L[h][pitch]                fp64: the last member's l, -inf where the prior masks the cell
//   part[h][nblk][2]           fp64: the block partials of the last launch's member rows
//   rows[member][h][2]         fp64: (mx, sum) over the cells of l + log prior, in add order
// One add is one group (one lag): k_origin_add, one thread per candidate cell, walks the findings in the order
// fixed at create -- those that can exclude a cell first -- gathers each v once and serves every amount of the
// group from it, and leaves the loop once every hypothesis of the cell is -inf; where a whole wave lies outside
// the intersected plumes the exit is uniform.  The same thread then updates its (A, S) -- one writer per cell, no
// atomics; -inf touches nothing -- and the block leaves its partial; k_origin_rows, one wave per hypothesis,
// adds the partials in the fixed order of origin_lane_sum.  The same calls give the same bits.  The accumulator
// is floating point: another order of adds or merges moves E = A + log S - log W within its stated bound.
// Known releases (ps_origin_set_known): the findings also catch the wasps of releases that are facts, not
// hypotheses.  Per member k_origin_background, one wave per known group on that lag's solver stream, leaves
// term[k][q] = fl(rak * v_k) of the group's releases; the last group's launch adds them in index order k to bg[q],
// forms the terms at mu = bg and one lane adds them in order q to the member's null row l0.  k_origin_add<true>
// then reads bg[q] -- the same for every lane -- and forms mu = bg + ra * v with two roundings; k_origin_add<false>
// is the code of a handle without known releases.
#include <math.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "ps_common.h"
#include "ps_origin_core.h"

#define PS_ORIGIN_ROWS0 64

namespace {

struct OrgSlots {   // rec nullptr (PS_REC_NONE): the group is not released yet on this day
  PsSrc s[PS_ORIGIN_MAX_SLOT];
};
struct OrgGroup {
  int nh, pad_;
  int h[PS_ORIGIN_MAX_HYP];    // the hypotheses of the group, ascending
};

__device__ inline double org_wave_max(double x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = fmax(x, __shfl_xor(x, m, 64));
  return x;
}
__device__ inline double org_wave_sum(double x) {   // a butterfly: every lane ends with the same bits
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = x + __shfl_xor(x, m, 64);
  return x;
}

struct OrgKnown {
  int n, last;                            // the group's releases; last: this launch also forms bg and l0
  int32_t k[PS_ORIGIN_MAX_KNOWN];         // their indices, ascending
  int32_t drow[PS_ORIGIN_MAX_KNOWN], dcol[PS_ORIGIN_MAX_KNOWN];
};

// One wave; lane q owns finding q (kernel order).  rak[k * nfind + q] = fl(rate * amount_k); term[k * nfind + q]
// is left by the launch of k's group, and read by the last group's launch: the same lane, or an earlier launch.
__global__ void __launch_bounds__(PS_ORIGIN_LANES)
    k_origin_background(OrgSlots desc, OrgKnown kn, const OriginFinding* __restrict__ find,
                        const double* __restrict__ rak, double* term, int nknown, int nfind, int N,
                        double* __restrict__ bg, double* __restrict__ null_row, double negval) {
  __shared__ double lterm[PS_ORIGIN_LANES];
  const int q = threadIdx.x;
  if (q < nfind) {
    const OriginFinding f = find[q];
    const PsSrc sd = desc.s[f.slot];
    const double delta = sd.rec && sd.stats ? sd.stats->delta : 0.0;
    for (int j = 0; j < kn.n; ++j) {
      double v = 0.0;
      int64_t src;
      if (sd.rec && origin_known_source(N, f.rowR, f.colR, kn.drow[j], kn.dcol[j], &src))
        v = ps_record_value(sd.rec[src], sd.stat_scale, sd.post_scale, delta, negval);
      term[(int64_t)kn.k[j] * nfind + q] = origin_bg_term(rak[(int64_t)kn.k[j] * nfind + q], v);
    }
    if (kn.last) {
      const double b = origin_bg_sum(term, nknown, nfind, q);
      bg[q] = b;
      lterm[q] = origin_term(f.kind, b, f.n, f.lgam);
    }
  }
  if (!kn.last) return;
  __syncthreads();
  if (q == 0) {
    const double l0 = origin_null_sum(lterm, nfind);
    *null_row = l0;
    bg[nfind] = l0;   // next to the background it belongs to: a merge appends null rows, not backgrounds
  }
}

// find, ra: the findings and the products rate_o * amount_h, ra[h * nfind + q], both in kernel order q; BG: bg[q],
// the background of finding q, is added to every mu
template <bool BG>
__global__ void __launch_bounds__(PS_ORIGIN_THREADS)
    k_origin_add(OrgSlots desc, OrgGroup grp, const OriginFinding* __restrict__ find, const double* __restrict__ ra,
                 const double* __restrict__ bg, int nfind, const double* __restrict__ prior, double* __restrict__ L,
                 double* __restrict__ A, double* __restrict__ S, double* __restrict__ part, int N, int64_t ncell,
                 int64_t pitch, int64_t nblk, double negval, double w) {
  __shared__ double smax[PS_ORIGIN_MAX_HYP][PS_ORIGIN_THREADS / 64];
  __shared__ double ssum[PS_ORIGIN_MAX_HYP][PS_ORIGIN_THREADS / 64];
  const int64_t i = blockIdx.x * (int64_t)PS_ORIGIN_THREADS + threadIdx.x;
  const bool in = i < ncell;
  const int r = in ? (int)(i / N) : 0, c = in ? (int)(i - (int64_t)r * N) : 0;
  const int nh = grp.nh;
  double lp = 0.0;
  bool alive = in;
  if (prior && in) {
    lp = prior[i];
    alive = lp != -INFINITY;   // a masked cell gathers nothing
  }
  double acc[PS_ORIGIN_MAX_HYP];
#pragma unroll
  for (int j = 0; j < PS_ORIGIN_MAX_HYP; ++j) acc[j] = alive ? 0.0 : -INFINITY;
  for (int q = 0; q < nfind; ++q) {
    if (!alive) break;
    const OriginFinding f = find[q];
    const PsSrc sd = desc.s[f.slot];
    double v = 0.0;
    int64_t src;
    if (sd.rec && origin_source(N, f.rowR, f.colR, r, c, &src)) {
      const double delta = sd.stats ? sd.stats->delta : 0.0;
      v = ps_record_value(sd.rec[src], sd.stat_scale, sd.post_scale, delta, negval);
    }
    const double bq = BG ? bg[q] : 0.0;
    bool any = false;
#pragma unroll
    for (int j = 0; j < PS_ORIGIN_MAX_HYP; ++j) {
      if (j < nh) {
        const double rav = ra[(int64_t)grp.h[j] * nfind + q];
        const double mu = BG ? origin_mu_bg(bq, rav, v) : rav * v;
        acc[j] = acc[j] + origin_term(f.kind, mu, f.n, f.lgam);
        any = any || acc[j] != -INFINITY;
      }
    }
    alive = any;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double y[PS_ORIGIN_MAX_HYP];
#pragma unroll
  for (int j = 0; j < PS_ORIGIN_MAX_HYP; ++j) {
    y[j] = -INFINITY;
    if (j < nh) {
      const double x = acc[j];
      if (in) {
        const int64_t at = (int64_t)grp.h[j] * pitch + i;
        L[at] = x;
        if (x != -INFINITY) {
          double a = A[at], s = S[at];
          origin_lse_add(&a, &s, x, w);
          A[at] = a;
          S[at] = s;
        }
      }
      y[j] = x + lp;             // -inf stays -inf: lp is finite wherever x is
      const double m = org_wave_max(y[j]);
      if (lane == 0) smax[j][wave] = m;
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < PS_ORIGIN_MAX_HYP; ++j) {
    if (j < nh) {
      double mb = smax[j][0];
#pragma unroll
      for (int k = 1; k < PS_ORIGIN_THREADS / 64; ++k) mb = fmax(mb, smax[j][k]);
      double e = 0.0;
      if (mb != -INFINITY) {     // uniform over the block
        e = y[j] == -INFINITY ? 0.0 : exp(y[j] - mb);
        e = org_wave_sum(e);
      }
      if (lane == 0) ssum[j][wave] = e;
    }
  }
  __syncthreads();
  if (threadIdx.x < nh) {
    const int j = threadIdx.x;
    double mb = smax[j][0], s = ssum[j][0];
    for (int k = 1; k < PS_ORIGIN_THREADS / 64; ++k) {
      mb = fmax(mb, smax[j][k]);
      s = s + ssum[j][k];        // the waves in index order
    }
    const int64_t at = origin_partial_at(grp.h[j], blockIdx.x, nblk);
    part[at] = mb;
    part[at + 1] = s;
  }
}

// blockIdx.x = the group's hypothesis j; one wave.  row: the member's row, [nhyp][2]
__global__ void __launch_bounds__(PS_ORIGIN_LANES)
    k_origin_rows(OrgGroup grp, const double* __restrict__ part, int64_t nblk, double* __restrict__ row) {
  __shared__ double lanes[PS_ORIGIN_LANES];
  const int h = grp.h[blockIdx.x], lane = threadIdx.x;
  const int64_t chunk = origin_chunk(nblk);
  const int64_t b0 = lane * chunk, b1 = b0 + chunk < nblk ? b0 + chunk : nblk;
  double mx = -INFINITY;
  for (int64_t b = b0; b < b1; ++b) mx = fmax(mx, part[origin_partial_at(h, b, nblk)]);
  mx = org_wave_max(mx);
  lanes[lane] = mx == -INFINITY ? 0.0 : origin_lane_sum(part, h, nblk, lane, mx);
  __syncthreads();
  if (lane == 0) {
    double s = 0.0;
    for (int l = 0; l < PS_ORIGIN_LANES; ++l) s = s + lanes[l];
    row[2 * h] = mx;
    row[2 * h + 1] = s;
  }
}

__global__ void k_origin_fill(double* __restrict__ A, double* __restrict__ S, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    A[i] = -INFINITY;
    S[i] = 0.0;
  }
}

__global__ void k_origin_merge(double* __restrict__ A, double* __restrict__ S, const double* __restrict__ A2,
                               const double* __restrict__ S2, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double x = A2[i];
    if (x == -INFINITY) continue;
    double a = A[i], s = S[i];
    origin_lse_add(&a, &s, x, S2[i]);
    A[i] = a;
    S[i] = s;
  }
}

}  // namespace

struct ps_origin {
  int device = 0, N = 0, nfind = 0, nslot = 0, nhyp = 0, ngroup = 0;
  int64_t ncell = 0, pitch = 0, nblk = 0;
  OrgGroup groups[PS_ORIGIN_MAX_GROUP];
  std::vector<int32_t> key_i;      // what two handles must share to merge: findings, hypotheses, slots
  std::vector<double> key_d;
  OriginFinding* find = nullptr;   // [nfind], kernel order
  double* ra = nullptr;            // [nhyp][nfind]
  double* prior = nullptr;         // [pitch] or nullptr: zeros
  double *A = nullptr, *S = nullptr, *L = nullptr;   // [nhyp][pitch]
  double* part = nullptr;          // [nhyp][nblk][2]
  double* rows = nullptr;          // [rows_cap][nhyp][2]
  int64_t rows_cap = 0;
  uint64_t W = 0;
  int64_t members = 0;
  std::vector<uint32_t> weights;   // per member, in row order
  int next_group = 0;              // the group the next add must name
  uint32_t pass_weight = 0;        // the weight group 0 of the pass under way came with
  // known releases (ps_origin_set_known); nknown == 0: none, and nothing below is allocated
  int nknown = 0, nk = 0;          // the releases and their groups (lags)
  OrgKnown kgroups[PS_ORIGIN_MAX_KGROUP];
  std::vector<int32_t> known_i;    // what two handles must share to merge: offsets and groups, amounts
  std::vector<double> known_d;
  std::vector<int32_t> order;      // order[q] = the finding, in the order given, that the kernel reads q-th
  std::vector<double> rate_q;      // the rates in kernel order
  double* rak = nullptr;           // [nknown][nfind] fl(rate * amount_k)
  double* term = nullptr;          // [nknown][nfind] the member's background terms
  double* bg = nullptr;            // [nfind + 1] the member's background, kernel order, and its l0
  double* null_rows = nullptr;     // [rows_cap] l0 per member, in add order
  int next_bg = 0;                 // the known group the next background call must name; nk: complete
  hipStream_t stream = nullptr;    // reset / merge / fetch / row growth
  PsLastOp last;                   // the last operation, on whatever stream it ran
  PsProf prof;                     // channel 0: the adds, 1: the rows, 2: the merges
};

static size_t org_plane_bytes(const ps_origin* p) { return (size_t)p->nhyp * p->pitch * sizeof(double); }
static size_t org_row_bytes(const ps_origin* p) { return (size_t)p->nhyp * 2 * sizeof(double); }
// the tables of the known releases: rak, term, bg
static size_t org_known_bytes(const ps_origin* p) {
  return p->nknown ? (((size_t)2 * p->nknown + 1) * p->nfind + 1) * sizeof(double) : 0;
}
static size_t org_fixed_bytes(const ps_origin* p, bool prior) {
  return 3 * org_plane_bytes(p) + (prior ? (size_t)p->pitch * sizeof(double) : 0) +
         (size_t)p->nhyp * p->nblk * 2 * sizeof(double) + (size_t)p->nfind * sizeof(OriginFinding) +
         (size_t)p->nhyp * p->nfind * sizeof(double) + org_known_bytes(p);
}
// a member under way holds a row (and a null row) past the members counted
static bool org_under_way(const ps_origin* p) { return p->next_group != 0 || p->next_bg != 0; }

// room for `need` member rows: a doubling copies the rows so far on the handle's stream and synchronises once
// before the old block is freed (as ps_range.hip)
static int org_reserve_rows(ps_origin* p, int64_t need) {
  if (need <= p->rows_cap) return PS_OK;
  int64_t cap = std::max<int64_t>(p->rows_cap, PS_ORIGIN_ROWS0);
  while (cap < need) cap *= 2;
  const size_t bytes = (size_t)cap * org_row_bytes(p);
  const size_t null_bytes = p->nknown ? (size_t)cap * sizeof(double) : 0;   // the null rows grow with the rows
  size_t free_b = 0, total_b = 0;
  PS_HIP(hipMemGetInfo(&free_b, &total_b));
  if (bytes + null_bytes > free_b)
    return ps_fail(PS_ERR_OOM, "origin: %lld member rows need %.3g GB, %.3g GB free", (long long)cap,
                   (double)(bytes + null_bytes) * 1e-9, (double)free_b * 1e-9);
  double *q = nullptr, *q0 = nullptr;
  PS_HIP(hipMalloc((void**)&q, bytes));
  if (null_bytes) {
    const hipError_t e0 = hipMalloc((void**)&q0, null_bytes);
    if (e0 != hipSuccess) {
      (void)hipFree(q);
      return ps_fail(PS_ERR_HIP, "origin: growing the null rows: %s", hipGetErrorString(e0));
    }
  }
  if (p->rows) {
    hipError_t e = hipSuccess;
    if (p->last.live) e = hipStreamWaitEvent(p->stream, p->last.ev, 0);
    const int64_t keep = p->members + (org_under_way(p) ? 1 : 0);   // the row of a pass under way too
    if (e == hipSuccess && keep > 0)
      e = hipMemcpyAsync(q, p->rows, (size_t)keep * org_row_bytes(p), hipMemcpyDeviceToDevice, p->stream);
    if (e == hipSuccess && keep > 0 && p->null_rows)
      e = hipMemcpyAsync(q0, p->null_rows, (size_t)keep * sizeof(double), hipMemcpyDeviceToDevice, p->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    if (e != hipSuccess) {
      (void)hipFree(q);
      if (q0) (void)hipFree(q0);
      return ps_fail(PS_ERR_HIP, "origin: growing the member rows: %s", hipGetErrorString(e));
    }
    PS_HIP(hipFree(p->rows));
    if (p->null_rows) PS_HIP(hipFree(p->null_rows));
  }
  p->rows = q;
  p->null_rows = q0;
  p->rows_cap = cap;
  return PS_OK;
}

extern "C" void ps_origin_destroy(ps_origin* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  p->last.sync();
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  p->prof.release();
  for (void* q : {(void*)p->find, (void*)p->ra, (void*)p->prior, (void*)p->A, (void*)p->S, (void*)p->L, (void*)p->part,
                  (void*)p->rows, (void*)p->rak, (void*)p->term, (void*)p->bg, (void*)p->null_rows})
    if (q) (void)hipFree(q);
  p->last.destroy();
  if (p->stream) (void)hipStreamDestroy(p->stream);
  delete p;
}

extern "C" int ps_origin_reset(ps_origin* p) {
  if (!p) return ps_fail(PS_ERR_BAD_ARG, "origin_reset: null handle");
  PS_HIP(hipSetDevice(p->device));
  PS_TRY(p->last.wait(p->stream));
  hipLaunchKernelGGL(k_origin_fill, dim3(1024), dim3(256), 0, p->stream, p->A, p->S, (int64_t)p->nhyp * p->pitch);
  PS_HIP(hipGetLastError());
  PS_TRY(p->last.mark(p->stream));
  p->W = 0;
  p->members = 0;
  p->weights.clear();
  p->next_group = 0;
  p->next_bg = 0;
  return PS_OK;
}

extern "C" int ps_origin_create(int device, int N, int nfind, const int32_t* row, const int32_t* col,
                                const int32_t* slot, const int32_t* kind, const double* rate, const double* n,
                                int nslot, int nhyp, const double* amount, const int32_t* hgroup, int ngroup,
                                const double* log_prior, ps_origin** out) {
  if (!out || N < 1 || (N & 1) == 0 || nfind < 1 || nfind > PS_ORIGIN_MAX_FIND || nslot < 1 ||
      nslot > PS_ORIGIN_MAX_SLOT || nhyp < 1 || nhyp > PS_ORIGIN_MAX_HYP || ngroup < 1 || ngroup > PS_ORIGIN_MAX_GROUP ||
      !row || !col || !slot || !kind || !rate || !n || !amount || !hgroup)
    return ps_fail(PS_ERR_BAD_ARG,
                   "origin_create: N %d (odd), %d findings (1..%d), %d days (1..%d), %d hypotheses (1..%d), %d groups "
                   "(1..%d)",
                   N, nfind, PS_ORIGIN_MAX_FIND, nslot, PS_ORIGIN_MAX_SLOT, nhyp, PS_ORIGIN_MAX_HYP, ngroup,
                   PS_ORIGIN_MAX_GROUP);
  *out = nullptr;
  for (int o = 0; o < nfind; ++o) {
    if (row[o] < 0 || row[o] >= N || col[o] < 0 || col[o] >= N)
      return ps_fail(PS_ERR_BAD_ARG, "origin_create: finding %d at cell (%d, %d) lies outside the %d x %d domain", o,
                     row[o], col[o], N, N);
    if (slot[o] < 0 || slot[o] >= nslot)
      return ps_fail(PS_ERR_BAD_ARG, "origin_create: finding %d reads day slot %d of %d", o, slot[o], nslot);
    if (kind[o] < PS_ORIGIN_COUNT || kind[o] > PS_ORIGIN_FOUND)
      return ps_fail(PS_ERR_BAD_ARG, "origin_create: finding %d has kind %d (0 count, 1 none, 2 found)", o, kind[o]);
    if (!isfinite(rate[o]) || !(rate[o] > 0.0))
      return ps_fail(PS_ERR_BAD_ARG, "origin_create: rate [%d] = %g is not finite and > 0", o, rate[o]);
    if (kind[o] == PS_ORIGIN_COUNT && !(n[o] >= 0.0 && n[o] <= 4294967295.0 && n[o] == floor(n[o])))
      return ps_fail(PS_ERR_BAD_ARG, "origin_create: the number found [%d] = %g is not a whole number >= 0", o, n[o]);
  }
  std::vector<int> per_group((size_t)ngroup, 0);
  for (int h = 0; h < nhyp; ++h) {
    if (!isfinite(amount[h]) || !(amount[h] > 0.0))
      return ps_fail(PS_ERR_BAD_ARG, "origin_create: amount %d = %g is not finite and > 0", h, amount[h]);
    if (hgroup[h] < 0 || hgroup[h] >= ngroup)
      return ps_fail(PS_ERR_BAD_ARG, "origin_create: hypothesis %d belongs to group %d of %d", h, hgroup[h], ngroup);
    per_group[(size_t)hgroup[h]] += 1;
  }
  for (int g = 0; g < ngroup; ++g)
    if (per_group[(size_t)g] == 0) return ps_fail(PS_ERR_BAD_ARG, "origin_create: group %d has no hypothesis", g);
  if (log_prior)
    for (int64_t i = 0; i < (int64_t)N * N; ++i)
      if (isnan(log_prior[i]) || log_prior[i] == INFINITY)
        return ps_fail(PS_ERR_BAD_ARG, "origin_create: the log-prior at cell %lld is %g (finite or -inf expected)",
                       (long long)i, log_prior[i]);
  PS_TRY(ps_use_device(device));
  ps_origin* p = new ps_origin();
  p->device = device;
  p->N = N;
  p->nfind = nfind;
  p->nslot = nslot;
  p->nhyp = nhyp;
  p->ngroup = ngroup;
  p->ncell = (int64_t)N * N;
  p->pitch = (p->ncell + 63) / 64 * 64;
  p->nblk = origin_nblk(p->ncell);
  auto fail = [&](int rc) {
    ps_origin_destroy(p);
    return rc;
  };
  if (p->nblk > 0x7fffffffLL) return fail(ps_fail(PS_ERR_BAD_ARG, "origin_create: N %d is too large for one launch", N));
  // everything but the member rows, checked before anything is allocated
  const double need = (double)org_fixed_bytes(p, log_prior != nullptr) + (double)PS_ORIGIN_ROWS0 * org_row_bytes(p);
  size_t free_b = 0, total_b = 0;
  hipError_t e = hipMemGetInfo(&free_b, &total_b);
  if (e != hipSuccess) return fail(ps_fail(PS_ERR_HIP, "origin_create: %s", hipGetErrorString(e)));
  if (need > (double)free_b)
    return fail(ps_fail(PS_ERR_OOM, "origin_create: %d hypotheses x 3 planes x %lld cells x 8 B and the tables = %.3g GB, "
                        "%.3g GB free", nhyp, (long long)p->pitch, need * 1e-9, (double)free_b * 1e-9));
  for (int g = 0; g < ngroup; ++g) {
    OrgGroup& G = p->groups[g];
    G = OrgGroup();
    for (int h = 0; h < nhyp; ++h)
      if (hgroup[h] == g) G.h[G.nh++] = h;
  }
  const int R = N / 2;
  std::vector<int32_t> order((size_t)nfind);
  origin_order(nfind, kind, n, order.data());
  std::vector<OriginFinding> find((size_t)nfind);
  std::vector<double> ra((size_t)nhyp * nfind);
  for (int q = 0; q < nfind; ++q) {
    const int o = order[(size_t)q];
    const double cnt = kind[o] == PS_ORIGIN_COUNT ? n[o] : 0.0;
    find[(size_t)q] = OriginFinding{row[o] + R, col[o] + R, slot[o], kind[o], cnt, lgamma(cnt + 1.0)};
    for (int h = 0; h < nhyp; ++h) ra[(size_t)h * nfind + q] = rate[o] * amount[h];   // formed once, here
    p->rate_q.push_back(rate[o]);
  }
  p->order = order;
  for (int o = 0; o < nfind; ++o) {
    p->key_i.insert(p->key_i.end(), {row[o], col[o], slot[o], kind[o]});
    p->key_d.insert(p->key_d.end(), {rate[o], kind[o] == PS_ORIGIN_COUNT ? n[o] : 0.0});
  }
  for (int h = 0; h < nhyp; ++h) {
    p->key_i.push_back(hgroup[h]);
    p->key_d.push_back(amount[h]);
  }
  p->key_i.push_back(nslot);
  const size_t pl = org_plane_bytes(p);
  e = hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = p->last.create();
  if (e == hipSuccess) e = hipMalloc((void**)&p->find, find.size() * sizeof(OriginFinding));
  if (e == hipSuccess) e = hipMalloc((void**)&p->ra, ra.size() * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&p->A, pl);
  if (e == hipSuccess) e = hipMalloc((void**)&p->S, pl);
  if (e == hipSuccess) e = hipMalloc((void**)&p->L, pl);
  if (e == hipSuccess) e = hipMalloc((void**)&p->part, (size_t)nhyp * p->nblk * 2 * sizeof(double));
  if (e == hipSuccess && log_prior) e = hipMalloc((void**)&p->prior, (size_t)p->pitch * sizeof(double));
  if (e == hipSuccess)
    e = hipMemcpyAsync(p->find, find.data(), find.size() * sizeof(OriginFinding), hipMemcpyHostToDevice, p->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(p->ra, ra.data(), ra.size() * sizeof(double), hipMemcpyHostToDevice, p->stream);
  if (e == hipSuccess && log_prior) {
    e = hipMemsetAsync(p->prior, 0, (size_t)p->pitch * sizeof(double), p->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(p->prior, log_prior, (size_t)p->ncell * sizeof(double), hipMemcpyHostToDevice, p->stream);
  }
  if (e == hipSuccess) e = hipMemsetAsync(p->L, 0, pl, p->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(p->stream);   // the host tables are read until here
  if (e != hipSuccess)
    return fail(ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "origin_create: %s", hipGetErrorString(e)));
  int rc = org_reserve_rows(p, PS_ORIGIN_ROWS0);
  if (rc == PS_OK) rc = ps_origin_reset(p);
  if (rc != PS_OK) return fail(rc);
  *out = p;
  return PS_OK;
}

extern "C" int ps_origin_reserve(ps_origin* p, int64_t members) {
  if (!p || members < 0) return ps_fail(PS_ERR_BAD_ARG, "origin_reserve: bad arguments");
  PS_HIP(hipSetDevice(p->device));
  return org_reserve_rows(p, members);
}

extern "C" int ps_origin_add(ps_origin* p, ps_solver* s, int group, int nslot, const int32_t* kind, const int32_t* idx,
                             const double* stat_scale, const double* post_scale, const int32_t* use_delta,
                             double negval, uint32_t weight) {
  if (!p || !s || !kind || !idx || !stat_scale || !post_scale || !use_delta)
    return ps_fail(PS_ERR_BAD_ARG, "origin_add: bad arguments");
  if (group < 0 || group >= p->ngroup) return ps_fail(PS_ERR_BAD_ARG, "origin_add: group %d of %d", group, p->ngroup);
  if (nslot != p->nslot) return ps_fail(PS_ERR_BAD_ARG, "origin_add: %d days given, the handle has %d", nslot, p->nslot);
  if (weight < 1) return ps_fail(PS_ERR_BAD_ARG, "origin_add: weight must be >= 1");
  if (group == 0 && p->next_group == 0 && !origin_backgrounds_done(p->next_bg, p->nk))
    return ps_fail(PS_ERR_STATE, "origin_add: the handle has known releases and background %d of %d of this member has "
                   "not come (ps_origin_background)", p->next_bg, p->nk);
  const int next = origin_next_group(p->next_group, group, p->ngroup);
  if (next < 0)
    return ps_fail(PS_ERR_STATE, "origin_add: group %d given, the member is at group %d (groups go 0 .. %d in order)",
                   group, p->next_group, p->ngroup - 1);
  if (group != 0 && weight != p->pass_weight)
    return ps_fail(PS_ERR_BAD_ARG, "origin_add: group %d comes with weight %u, group 0 of this member came with %u", group,
                   weight, p->pass_weight);
  if (group == 0 && p->W + weight > 0xffffffffull)
    return ps_fail(PS_ERR_BAD_ARG, "origin_add: total weight %llu would pass 2^32 - 1",
                   (unsigned long long)(p->W + weight));
  PS_HIP(hipSetDevice(p->device));
  // every descriptor first: an add with a bad record enqueues nothing
  OrgSlots desc;
  hipStream_t stream = nullptr;
  bool any = false;
  PS_TRY(ps_read_records("origin_add", "handle", p->device, p->N, s, nslot, kind, idx, stat_scale, post_scale,
                         use_delta, true, desc.s, &stream, &any));
  for (int e = nslot; e < PS_ORIGIN_MAX_SLOT; ++e) desc.s[e] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  if (!any)   // such a lag explains no finding, and no record names the stream to run on
    return ps_fail(PS_ERR_BAD_ARG, "origin_add: group %d is released on no day of a finding (every slot is PS_REC_NONE)",
                   group);
  if (group == 0) PS_TRY(org_reserve_rows(p, p->members + 1));
  PS_TRY(p->last.wait(stream));
  const OrgGroup& G = p->groups[group];
  hipEvent_t e1 = nullptr;
  PS_TRY(p->prof.begin(0, stream, &e1));
  if (p->nknown)
    hipLaunchKernelGGL(k_origin_add<true>, dim3((unsigned)p->nblk), dim3(PS_ORIGIN_THREADS), 0, stream, desc, G, p->find,
                       p->ra, p->bg, p->nfind, p->prior, p->L, p->A, p->S, p->part, p->N, p->ncell, p->pitch, p->nblk,
                       negval, (double)weight);
  else
    hipLaunchKernelGGL(k_origin_add<false>, dim3((unsigned)p->nblk), dim3(PS_ORIGIN_THREADS), 0, stream, desc, G, p->find,
                       p->ra, (const double*)nullptr, p->nfind, p->prior, p->L, p->A, p->S, p->part, p->N, p->ncell,
                       p->pitch, p->nblk, negval, (double)weight);
  PS_HIP(hipGetLastError());
  PS_TRY(p->prof.end(stream, e1));
  PS_TRY(p->prof.begin(1, stream, &e1));
  hipLaunchKernelGGL(k_origin_rows, dim3(G.nh), dim3(PS_ORIGIN_LANES), 0, stream, G, p->part, p->nblk,
                     p->rows + p->members * p->nhyp * 2);
  PS_HIP(hipGetLastError());
  PS_TRY(p->prof.end(stream, e1));
  PS_TRY(p->last.mark(stream));
  if (group == 0) p->pass_weight = weight;
  p->next_group = next;
  if (next == 0) {   // the member counts once its last group is in
    p->next_bg = 0;
    p->W += weight;
    p->members += 1;
    p->weights.push_back(weight);
  }
  return PS_OK;
}

extern "C" int ps_origin_set_known(ps_origin* p, int nknown, const int32_t* drow, const int32_t* dcol,
                                   const double* amount, const int32_t* kgroup, int nkgroup) {
  if (!p || !drow || !dcol || !amount || !kgroup || nknown < 1 || nknown > PS_ORIGIN_MAX_KNOWN || nkgroup < 1 ||
      nkgroup > PS_ORIGIN_MAX_KGROUP)
    return ps_fail(PS_ERR_BAD_ARG, "origin_set_known: %d known releases (1..%d), %d known groups (1..%d)", nknown,
                   PS_ORIGIN_MAX_KNOWN, nkgroup, PS_ORIGIN_MAX_KGROUP);
  if (p->nknown) return ps_fail(PS_ERR_STATE, "origin_set_known: the handle has its %d known releases already", p->nknown);
  if (p->members != 0 || p->next_group != 0)
    return ps_fail(PS_ERR_STATE, "origin_set_known: the known releases come before the first member (%lld are in)",
                   (long long)p->members + (p->next_group != 0 ? 1 : 0));
  std::vector<int> per_group((size_t)nkgroup, 0);
  for (int k = 0; k < nknown; ++k) {
    if (!isfinite(amount[k]) || !(amount[k] > 0.0))
      return ps_fail(PS_ERR_BAD_ARG, "origin_set_known: amount %d = %g is not finite and > 0", k, amount[k]);
    if (drow[k] <= -p->N || drow[k] >= p->N || dcol[k] <= -p->N || dcol[k] >= p->N)
      return ps_fail(PS_ERR_BAD_ARG, "origin_set_known: known release %d at offset (%d, %d) lies beyond the %d x %d domain",
                     k, drow[k], dcol[k], p->N, p->N);
    if (kgroup[k] < 0 || kgroup[k] >= nkgroup)
      return ps_fail(PS_ERR_BAD_ARG, "origin_set_known: known release %d belongs to known group %d of %d", k, kgroup[k],
                     nkgroup);
    per_group[(size_t)kgroup[k]] += 1;
  }
  for (int g = 0; g < nkgroup; ++g)
    if (per_group[(size_t)g] == 0)
      return ps_fail(PS_ERR_BAD_ARG, "origin_set_known: known group %d has no release", g);
  PS_HIP(hipSetDevice(p->device));
  std::vector<double> rak((size_t)nknown * p->nfind);
  for (int k = 0; k < nknown; ++k)
    for (int q = 0; q < p->nfind; ++q) rak[(size_t)k * p->nfind + q] = p->rate_q[(size_t)q] * amount[k];   // once, here
  const size_t tb = rak.size() * sizeof(double);
  double *d_rak = nullptr, *d_term = nullptr, *d_bg = nullptr, *d_null = nullptr;
  hipError_t e = hipMalloc((void**)&d_rak, tb);
  if (e == hipSuccess) e = hipMalloc((void**)&d_term, tb);
  if (e == hipSuccess) e = hipMalloc((void**)&d_bg, ((size_t)p->nfind + 1) * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&d_null, (size_t)p->rows_cap * sizeof(double));
  if (e == hipSuccess) e = p->last.live ? hipStreamWaitEvent(p->stream, p->last.ev, 0) : hipSuccess;
  if (e == hipSuccess) e = hipMemcpyAsync(d_rak, rak.data(), tb, hipMemcpyHostToDevice, p->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_term, 0, tb, p->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_bg, 0, ((size_t)p->nfind + 1) * sizeof(double), p->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(p->stream);   // the host table is read until here
  if (e != hipSuccess) {
    for (void* q : {(void*)d_rak, (void*)d_term, (void*)d_bg, (void*)d_null})
      if (q) (void)hipFree(q);
    return ps_fail(e == hipErrorOutOfMemory ? PS_ERR_OOM : PS_ERR_HIP, "origin_set_known: %s", hipGetErrorString(e));
  }
  p->rak = d_rak;
  p->term = d_term;
  p->bg = d_bg;
  p->null_rows = d_null;
  for (int g = 0; g < nkgroup; ++g) {
    OrgKnown& G = p->kgroups[g];
    G = OrgKnown();
    G.last = g + 1 == nkgroup;
    for (int k = 0; k < nknown; ++k)
      if (kgroup[k] == g) {
        G.k[G.n] = k;
        G.drow[G.n] = drow[k];
        G.dcol[G.n] = dcol[k];
        G.n += 1;
      }
  }
  for (int k = 0; k < nknown; ++k) {
    p->known_i.insert(p->known_i.end(), {drow[k], dcol[k], kgroup[k]});
    p->known_d.push_back(amount[k]);
  }
  p->nknown = nknown;
  p->nk = nkgroup;
  p->next_bg = 0;
  return PS_OK;
}

extern "C" int ps_origin_background(ps_origin* p, ps_solver* s, int kgroup, int nslot, const int32_t* kind,
                                    const int32_t* idx, const double* stat_scale, const double* post_scale,
                                    const int32_t* use_delta, double negval) {
  if (!p || !s || !kind || !idx || !stat_scale || !post_scale || !use_delta)
    return ps_fail(PS_ERR_BAD_ARG, "origin_background: bad arguments");
  if (!p->nknown) return ps_fail(PS_ERR_STATE, "origin_background: the handle has no known releases (ps_origin_set_known)");
  if (kgroup < 0 || kgroup >= p->nk)
    return ps_fail(PS_ERR_BAD_ARG, "origin_background: known group %d of %d", kgroup, p->nk);
  if (nslot != p->nslot)
    return ps_fail(PS_ERR_BAD_ARG, "origin_background: %d days given, the handle has %d", nslot, p->nslot);
  const int next = origin_next_background(p->next_bg, p->next_group, kgroup, p->nk);
  if (next < 0) {
    if (p->next_group != 0)
      return ps_fail(PS_ERR_STATE, "origin_background: the adds of a member are under way (group %d of %d is next)",
                     p->next_group, p->ngroup);
    return ps_fail(PS_ERR_STATE, "origin_background: known group %d given, the member is at known group %d of %d (they "
                   "go 0 .. %d in order, then the adds)", kgroup, p->next_bg, p->nk, p->nk - 1);
  }
  PS_HIP(hipSetDevice(p->device));
  // every descriptor first: a call with a bad record enqueues nothing
  OrgSlots desc;
  hipStream_t stream = p->stream;   // a known group released after every finding reads no record: the handle's stream
  PS_TRY(ps_read_records("origin_background", "handle", p->device, p->N, s, nslot, kind, idx, stat_scale, post_scale,
                         use_delta, true, desc.s, &stream));
  for (int e = nslot; e < PS_ORIGIN_MAX_SLOT; ++e) desc.s[e] = PsSrc{nullptr, nullptr, 0.0, 0.0};
  if (kgroup == 0) PS_TRY(org_reserve_rows(p, p->members + 1));
  PS_TRY(p->last.wait(stream));
  hipLaunchKernelGGL(k_origin_background, dim3(1), dim3(PS_ORIGIN_LANES), 0, stream, desc, p->kgroups[kgroup], p->find,
                     p->rak, p->term, p->nknown, p->nfind, p->N, p->bg, p->null_rows + p->members, negval);
  PS_HIP(hipGetLastError());
  PS_TRY(p->last.mark(stream));
  p->next_bg = next;
  return PS_OK;
}

extern "C" int ps_origin_fetch_background(ps_origin* p, double* bg, double* l0) {
  if (!p) return ps_fail(PS_ERR_BAD_ARG, "origin_fetch_background: null handle");
  if (!p->nknown) return ps_fail(PS_ERR_STATE, "origin_fetch_background: the handle has no known releases");
  if (p->members == 0) return ps_fail(PS_ERR_STATE, "origin_fetch_background: no member added yet");
  if (org_under_way(p)) return ps_fail(PS_ERR_STATE, "origin_fetch_background: a member is under way");
  PS_HIP(hipSetDevice(p->device));
  PS_TRY(p->last.wait(p->stream));
  double q[PS_ORIGIN_MAX_FIND + 1];
  PS_HIP(hipMemcpyAsync(q, p->bg, ((size_t)p->nfind + 1) * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  PS_HIP(hipStreamSynchronize(p->stream));
  if (bg)
    for (int k = 0; k < p->nfind; ++k) bg[p->order[(size_t)k]] = q[k];   // back to the order given
  if (l0) *l0 = q[p->nfind];
  return PS_OK;
}

extern "C" int ps_origin_null_rows(ps_origin* p, int64_t members_expected, double* rows) {
  if (!p) return ps_fail(PS_ERR_BAD_ARG, "origin_null_rows: null handle");
  if (!p->nknown) return ps_fail(PS_ERR_STATE, "origin_null_rows: the handle has no known releases");
  if (members_expected != p->members)
    return ps_fail(PS_ERR_BAD_ARG, "origin_null_rows: room for %lld members given, the handle holds %lld",
                   (long long)members_expected, (long long)p->members);
  if (p->members == 0 || !rows) return PS_OK;
  PS_HIP(hipSetDevice(p->device));
  PS_TRY(p->last.wait(p->stream));
  PS_HIP(hipMemcpyAsync(rows, p->null_rows, (size_t)p->members * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  PS_HIP(hipStreamSynchronize(p->stream));
  return PS_OK;
}

static bool org_same(const ps_origin* a, const ps_origin* b) {
  return a->device == b->device && a->N == b->N && a->key_i == b->key_i && a->key_d == b->key_d &&
         (a->prior == nullptr) == (b->prior == nullptr);
}
static bool org_same_known(const ps_origin* a, const ps_origin* b) {
  return a->nknown == b->nknown && a->nk == b->nk && a->known_i == b->known_i && a->known_d == b->known_d;
}

extern "C" int ps_origin_merge(ps_origin* dst, ps_origin* src) {
  if (!dst || !src || dst == src) return ps_fail(PS_ERR_BAD_ARG, "origin_merge: bad arguments");
  if (dst->device != src->device)
    return ps_fail(PS_ERR_BAD_ARG, "origin_merge: handles on devices %d and %d", dst->device, src->device);
  if (dst->N != src->N) return ps_fail(PS_ERR_BAD_ARG, "origin_merge: domains %d and %d", dst->N, src->N);
  if (!org_same(dst, src))
    return ps_fail(PS_ERR_BAD_ARG, "origin_merge: handles differ in findings, hypotheses, days or prior");
  if (!org_same_known(dst, src))
    return ps_fail(PS_ERR_BAD_ARG, "origin_merge: handles differ in their known releases (%d and %d of them)",
                   dst->nknown, src->nknown);
  if (dst->next_group != 0 || src->next_group != 0)
    return ps_fail(PS_ERR_STATE, "origin_merge: a member is under way (group %d of %d is next)",
                   dst->next_group ? dst->next_group : src->next_group, dst->ngroup);
  if (dst->next_bg != 0 || src->next_bg != 0)
    return ps_fail(PS_ERR_STATE, "origin_merge: a member is under way (its backgrounds are in, its adds are not)");
  if (dst->W + src->W > 0xffffffffull) return ps_fail(PS_ERR_BAD_ARG, "origin_merge: total weight would pass 2^32 - 1");
  if (src->members == 0) return PS_OK;
  PS_HIP(hipSetDevice(dst->device));
  PS_TRY(org_reserve_rows(dst, dst->members + src->members));
  PS_TRY(dst->last.wait(dst->stream));
  PS_TRY(src->last.wait(dst->stream));
  hipEvent_t e1 = nullptr;
  PS_TRY(dst->prof.begin(2, dst->stream, &e1));
  hipLaunchKernelGGL(k_origin_merge, dim3(1024), dim3(256), 0, dst->stream, dst->A, dst->S, src->A, src->S,
                     (int64_t)dst->nhyp * dst->pitch);
  PS_HIP(hipGetLastError());
  PS_TRY(dst->prof.end(dst->stream, e1));
  PS_HIP(hipMemcpyAsync(dst->rows + dst->members * dst->nhyp * 2, src->rows, (size_t)src->members * org_row_bytes(src),
                        hipMemcpyDeviceToDevice, dst->stream));
  if (dst->nknown)
    PS_HIP(hipMemcpyAsync(dst->null_rows + dst->members, src->null_rows, (size_t)src->members * sizeof(double),
                          hipMemcpyDeviceToDevice, dst->stream));
  PS_TRY(dst->last.mark(dst->stream));
  PS_TRY(src->last.mark(dst->stream));   // src is read until then
  dst->W += src->W;
  dst->members += src->members;
  dst->weights.insert(dst->weights.end(), src->weights.begin(), src->weights.end());
  return PS_OK;
}

extern "C" int ps_origin_fetch(ps_origin* p, int what, int h, double* out) {
  if (!p || !out) return ps_fail(PS_ERR_BAD_ARG, "origin_fetch: bad arguments");
  if (what < 0 || what > 2) return ps_fail(PS_ERR_BAD_ARG, "origin_fetch: plane %d (0 A, 1 S, 2 the last member's l)", what);
  if (h < 0 || h >= p->nhyp) return ps_fail(PS_ERR_BAD_ARG, "origin_fetch: hypothesis %d of %d", h, p->nhyp);
  if (p->members == 0) return ps_fail(PS_ERR_STATE, "origin_fetch: no member added yet");
  if (org_under_way(p))
    return ps_fail(PS_ERR_STATE, "origin_fetch: group %d of %d of the current member has not been added", p->next_group,
                   p->ngroup);
  PS_HIP(hipSetDevice(p->device));
  PS_TRY(p->last.wait(p->stream));
  const double* src = (what == 0 ? p->A : what == 1 ? p->S : p->L) + (int64_t)h * p->pitch;
  PS_HIP(hipMemcpyAsync(out, src, (size_t)p->ncell * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  PS_HIP(hipStreamSynchronize(p->stream));
  return PS_OK;
}

extern "C" int ps_origin_members(ps_origin* p, int64_t members_expected, double* rows, uint32_t* weights) {
  if (!p) return ps_fail(PS_ERR_BAD_ARG, "origin_members: null handle");
  if (members_expected != p->members)
    return ps_fail(PS_ERR_BAD_ARG, "origin_members: room for %lld members given, the handle holds %lld",
                   (long long)members_expected, (long long)p->members);
  if (p->members == 0) return PS_OK;
  if (weights) std::copy(p->weights.begin(), p->weights.end(), weights);
  if (rows) {
    PS_HIP(hipSetDevice(p->device));
    PS_TRY(p->last.wait(p->stream));
    PS_HIP(hipMemcpyAsync(rows, p->rows, (size_t)p->members * org_row_bytes(p), hipMemcpyDeviceToHost, p->stream));
    PS_HIP(hipStreamSynchronize(p->stream));
  }
  return PS_OK;
}

extern "C" int ps_origin_info(ps_origin* p, double* total_weight, int64_t* members, int64_t* capacity, int64_t* bytes) {
  if (!p) return ps_fail(PS_ERR_BAD_ARG, "origin_info: null handle");
  if (total_weight) *total_weight = (double)p->W;
  if (members) *members = p->members;
  if (capacity) *capacity = p->rows_cap;
  if (bytes) *bytes = (int64_t)(org_fixed_bytes(p, p->prior != nullptr) + (size_t)p->rows_cap * org_row_bytes(p) +
                             (p->nknown ? (size_t)p->rows_cap * sizeof(double) : 0));
  return PS_OK;
}

extern "C" int ps_origin_prof(ps_origin* p, int enable, double* add_ms, int64_t* adds, double* rows_ms, int64_t* rows_n,
                              double* merge_ms, int64_t* merges) {
  if (!p) return ps_fail(PS_ERR_BAD_ARG, "origin_prof: null handle");
  PS_HIP(hipSetDevice(p->device));
  p->prof.set(enable);
  double* ms[3] = {add_ms, rows_ms, merge_ms};
  int64_t* cnt[3] = {adds, rows_n, merges};
  for (int k = 0; k < 3; ++k)
    if (ms[k] || cnt[k]) PS_TRY(p->prof.totals(k, ms[k], cnt[k]));
  return PS_OK;
}
