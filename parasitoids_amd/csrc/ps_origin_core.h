// The per-thread logic of the origin maps (ps_origin.hip): where a candidate origin reads a finding's record, the
// order the findings are summed in, one finding's log-likelihood term, the streaming log-sum-exp pair (A, S), the
// order of a member's groups, and the layout and order of the member rows' two-stage reduction.  Plain C++ that
// compiles for host and device: the kernels and the host emulation (tests/host/origin_emul.cpp) share it.
//   a release at cell s = (r, c) instead of the centre (R, R) moves the field by (r - R, c - R), so the finding
//   at (fr, fc) sees what the centre release holds at (fr + R - r, fc + R - c); outside [0, N) on either axis
//   it sees 0, per axis and never by the flat index (nothing wraps, as ps_sites.hip)
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef PS_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PS_HD __host__ __device__ __forceinline__
#else
#define PS_HD inline
#endif
#endif

#define PS_ORIGIN_MAX_FIND 64
#define PS_ORIGIN_MAX_HYP 8
#define PS_ORIGIN_MAX_GROUP 4
#define PS_ORIGIN_MAX_SLOT 32    // distinct days: one launch's descriptors, 32 x 32 B of kernel arguments
#define PS_ORIGIN_THREADS 256    // one block of the likelihood kernel: one cell per thread, one partial per block
#define PS_ORIGIN_LANES 64       // the row reduction: one wave per hypothesis

#define PS_ORIGIN_COUNT 0        // n found: n log(mu) - mu - lgamma(n + 1); at mu = 0: 0 if n == 0 else -inf
#define PS_ORIGIN_NONE 1         // looked, nothing found: -mu
#define PS_ORIGIN_FOUND 2        // at least one found: log(1 - exp(-mu)); at mu = 0: -inf

// one finding as the kernel reads it: the same for every lane
struct OriginFinding {
  int32_t rowR, colR;            // the finding's cell plus R on either axis
  int32_t slot, kind;
  double n, lgam;                // the number found and lgamma(n + 1), 0 for the other kinds
};

// the source cell of finding (rowR, colR) for the candidate (r, c); false where it leaves the domain
PS_HD bool origin_source(int N, int rowR, int colR, int r, int c, int64_t* src) {
  const int rs = rowR - r, cs = colR - c;
  const bool ok = (unsigned)rs < (unsigned)N && (unsigned)cs < (unsigned)N;
  *src = ok ? (int64_t)rs * N + cs : 0;
  return ok;
}

// can the finding make a cell -inf?  a positive count or a 'found' at mu = 0
PS_HD bool origin_can_exclude(int kind, double n) {
  return kind == PS_ORIGIN_FOUND || (kind == PS_ORIGIN_COUNT && n > 0.0);
}

// the kernel's order of the findings: those that can exclude a cell first, each class in the order given
inline void origin_order(int nfind, const int32_t* kind, const double* n, int32_t* order) {
  int q = 0;
  for (int pass = 0; pass < 2; ++pass)
    for (int o = 0; o < nfind; ++o)
      if (origin_can_exclude(kind[o], n[o]) == (pass == 0)) order[q++] = o;
}

// one finding's term at mu >= 0
PS_HD double origin_term(int kind, double mu, double n, double lgam) {
  if (kind == PS_ORIGIN_NONE || (kind == PS_ORIGIN_COUNT && n == 0.0)) return -mu;
  if (mu == 0.0) return -INFINITY;
  if (kind == PS_ORIGIN_FOUND) return mu <= 0.6931471805599453 ? log(-expm1(-mu)) : log1p(-exp(-mu));
  return n * log(mu) - mu - lgam;
}

// (A, S) takes a term of log-value x and mass w > 0: afterwards A is the larger log-value and S the masses in
// units of exp(A).  The same rule adds a member (w its weight) and merges two pairs (x, w the other pair).
PS_HD void origin_lse_add(double* A, double* S, double x, double w) {
  if (x == -INFINITY) return;
  if (*A == -INFINITY) {
    *A = x;
    *S = w;
  } else if (x <= *A) {
    *S = *S + w * exp(x - *A);
  } else {
    *S = *S * exp(*A - x) + w;
    *A = x;
  }
}

// the group the pass expects after `group` of `ngroup`; -1 where `group` may not come now.  Unlike a release
// plan, group 0 may not come early: the groups already in have changed (A, S), so a pass cannot be abandoned.
PS_HD int origin_next_group(int next, int group, int ngroup) {
  if (group < 0 || group >= ngroup || group != next) return -1;
  return group + 1 == ngroup ? 0 : group + 1;
}

// ---- known releases in the background (ps_origin_set_known) ----
#define PS_ORIGIN_MAX_KNOWN 32
#define PS_ORIGIN_MAX_KGROUP 4

// what finding (rowR, colR) sees of the known release k, drow / dcol cells off the centre: the centre release's
// field at (r_o - drow, c_o - dcol), which is origin_source for the candidate cell (R + drow, R + dcol)
PS_HD bool origin_known_source(int N, int rowR, int colR, int drow, int dcol, int64_t* src) {
  const int R = N / 2;
  return origin_source(N, rowR, colR, R + drow, R + dcol, src);
}

// one term of the background: fl(rak * v), rak = fl(rate_o * amount_k) formed on the host
PS_HD double origin_bg_term(double rak, double v) { return rak * v; }

// bg of one finding: the terms term[k * nfind + q] of every known release in index order, from +0.0
PS_HD double origin_bg_sum(const double* term, int nknown, int nfind, int q) {
  double s = 0.0;
  for (int k = 0; k < nknown; ++k) {
    const double t = term[(int64_t)k * nfind + q];
    s = s + t;
  }
  return s;
}

// mu of candidate and hypothesis over a background: the product and the sum rounded separately
PS_HD double origin_mu_bg(double bg, double ra, double v) {
  const double t = ra * v;
  const double mu = bg + t;
  return mu;
}

// the null row: the terms at mu = bg in the kernel's order q, from +0.0
PS_HD double origin_null_sum(const double* term, int nfind) {
  double s = 0.0;
  for (int q = 0; q < nfind; ++q) s = s + term[q];
  return s;
}

// One member of a handle with nk known groups: the background calls 0 .. nk - 1 in order, then the adds.  next_bg
// counts the background calls in (nk: complete), next_group is that of origin_next_group.  -> next_bg after the
// background call for known group g, or -1 where it may not come now: out of order, after the backgrounds are
// complete, or while the adds of a member are under way.
PS_HD int origin_next_background(int next_bg, int next_group, int g, int nk) {
  if (g < 0 || g >= nk || next_group != 0 || g != next_bg) return -1;
  return g + 1;
}
// may group 0 of the adds come?  a handle without known releases: always; with: once the backgrounds are complete
PS_HD bool origin_backgrounds_done(int next_bg, int nk) { return next_bg == nk; }

// the member rows.  Stage one: block b of the likelihood launch owns the cells b * THREADS .. and leaves, per
// hypothesis h, partial[(h * nblk + b) * 2 + {0, 1}] = (max, sum of exp(x - max)) of its cells.  Stage two: one
// wave per hypothesis; lane l owns the partials l * chunk .. min((l + 1) * chunk, nblk) - 1 and adds them in
// index order, lane 0 then adds the lanes' sums in lane order.
PS_HD int64_t origin_nblk(int64_t ncell) { return (ncell + PS_ORIGIN_THREADS - 1) / PS_ORIGIN_THREADS; }
PS_HD int64_t origin_partial_at(int h, int64_t b, int64_t nblk) { return ((int64_t)h * nblk + b) * 2; }
PS_HD int64_t origin_chunk(int64_t nblk) { return (nblk + PS_ORIGIN_LANES - 1) / PS_ORIGIN_LANES; }

// a lane's share of stage two, given the maximum over all partials
PS_HD double origin_lane_sum(const double* part, int h, int64_t nblk, int lane, double mx) {
  const int64_t chunk = origin_chunk(nblk);
  int64_t b0 = lane * chunk, b1 = b0 + chunk;
  if (b1 > nblk) b1 = nblk;
  double s = 0.0;
  for (int64_t b = b0; b < b1; ++b) {
    const int64_t at = origin_partial_at(h, b, nblk);
    if (part[at] != -INFINITY) s = s + part[at + 1] * exp(part[at] - mx);
  }
  return s;
}
