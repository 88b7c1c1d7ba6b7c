// Host emulation of the origin maps' device logic (csrc/ps_origin_core.h): the shifted read of every finding for
// every candidate cell, the kernel's order of the findings, the order of a member's groups, the streaming (A, S)
// pair and both stages of the member rows in the layout of the device, on 8 threads that each own whole blocks --
// against a brute force that moves the field to the candidate and reads it at the finding.  Findings in all four
// corners and at the centre, so the shifted reads leave the domain on every side.  Prints "ok <cases>" or
// "FAIL ..." and exits 1.
//   origin_emul N [N ...]
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <thread>
#include <vector>

#include "../../parasitoids_amd/csrc/ps_origin_core.h"

static const int NTHREAD = 8;

template <class F>
static void on_threads(int64_t n, F body) {
  std::vector<std::thread> pool;
  for (int t = 0; t < NTHREAD; ++t)
    pool.emplace_back([=] {
      for (int64_t i = t; i < n; i += NTHREAD) body(i);
    });
  for (auto& th : pool) th.join();
}

static int fail(const char* what, int N, long long a, long long b) {
  printf("FAIL %s at N = %d: %lld %lld\n", what, N, a, b);
  return 1;
}

// a blob off the centre with exact zeros around it, a few holes inside
static std::vector<double> make_field(int N, int which) {
  std::vector<double> f((size_t)N * N, 0.0);
  uint64_t s = 0x9e3779b97f4a7c15ull * (uint64_t)(N + 7 * which + 1);
  const int cy = N / 2 + (which ? -N / 5 : N / 7), cx = N / 2 + (which ? N / 6 : -N / 9), rad = N / 3 + which;
  for (int y = 0; y < N; ++y)
    for (int x = 0; x < N; ++x) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      const int d2 = (y - cy) * (y - cy) + (x - cx) * (x - cx);
      if (d2 <= rad * rad && (s >> 60) != 0) f[(size_t)y * N + x] = 5.0 * exp(-d2 / (0.3 * rad * rad)) + 1e-3;
    }
  return f;
}

static int run_size(int N, int* cases) {
  const int R = N / 2, nhyp = 3, nfind = 7;
  const int64_t ncell = (int64_t)N * N, nblk = origin_nblk(ncell);
  // findings: the four corners (they exclude nothing, but their reads leave the domain on every side), the centre
  // and two more that can exclude a cell; every kind, a count of 0 among them
  const int32_t row[nfind] = {0, 0, N - 1, N - 1, R, R - R / 4, R + R / 3};
  const int32_t col[nfind] = {0, N - 1, 0, N - 1, R, R + R / 3, R + R / 4};
  const int32_t kind[nfind] = {PS_ORIGIN_NONE, PS_ORIGIN_COUNT, PS_ORIGIN_NONE, PS_ORIGIN_NONE,
                               PS_ORIGIN_COUNT, PS_ORIGIN_COUNT, PS_ORIGIN_FOUND};
  const double cnt[nfind] = {0, 0, 0, 0, 3, 1, 0};
  const double rate[nfind] = {0.5, 0.25, 1.0, 0.125, 0.5, 2.0, 0.75};
  const double amount[nhyp] = {0.1, 1.0, 10.0};
  int32_t order[nfind];
  origin_order(nfind, kind, cnt, order);
  const int32_t want_order[nfind] = {4, 5, 6, 0, 1, 2, 3};
  for (int q = 0; q < nfind; ++q)
    if (order[q] != want_order[q]) return fail("order", N, q, order[q]);
  std::vector<OriginFinding> find(nfind);
  for (int q = 0; q < nfind; ++q) {
    const int o = order[q];
    find[q] = OriginFinding{row[o] + R, col[o] + R, 0, kind[o], cnt[o], lgamma(cnt[o] + 1.0)};
  }
  std::vector<double> A((size_t)nhyp * ncell, -INFINITY), S((size_t)nhyp * ncell, 0.0);
  std::vector<double> lse_ref((size_t)nhyp * ncell, 0.0);   // sum of w exp(l) per cell, directly
  const double weights[2] = {1.0, 3.0};
  for (int member = 0; member < 2; ++member) {
    const std::vector<double> field = make_field(N, member);
    std::vector<double> L((size_t)nhyp * ncell, NAN), part((size_t)nhyp * nblk * 2, NAN);
    // the kernel: block b owns cells b * THREADS .., one emulated thread per cell
    on_threads(nblk, [&](int64_t b) {
      double bmax[nhyp], bsum[nhyp];
      std::vector<double> x((size_t)nhyp * PS_ORIGIN_THREADS, -INFINITY);
      for (int t = 0; t < PS_ORIGIN_THREADS; ++t) {
        const int64_t i = b * PS_ORIGIN_THREADS + t;
        if (i >= ncell) continue;
        const int r = (int)(i / N), c = (int)(i - (int64_t)r * N);
        double acc[nhyp] = {0.0, 0.0, 0.0};
        bool alive = true;
        for (int q = 0; q < nfind && alive; ++q) {
          int64_t src;
          double v = 0.0;
          if (origin_source(N, find[q].rowR, find[q].colR, r, c, &src)) v = field[(size_t)src];   // ASan watches src
          bool any = false;
          for (int h = 0; h < nhyp; ++h) {
            const double mu = (rate[order[q]] * amount[h]) * v;
            acc[h] = acc[h] + origin_term(find[q].kind, mu, find[q].n, find[q].lgam);
            any = any || acc[h] != -INFINITY;
          }
          alive = any;
        }
        for (int h = 0; h < nhyp; ++h) {
          L[(size_t)h * ncell + i] = acc[h];
          x[(size_t)h * PS_ORIGIN_THREADS + t] = acc[h];
          origin_lse_add(&A[(size_t)h * ncell + i], &S[(size_t)h * ncell + i], acc[h], weights[member]);
        }
      }
      for (int h = 0; h < nhyp; ++h) {
        bmax[h] = -INFINITY;
        bsum[h] = 0.0;
        for (int t = 0; t < PS_ORIGIN_THREADS; ++t) bmax[h] = fmax(bmax[h], x[(size_t)h * PS_ORIGIN_THREADS + t]);
        if (bmax[h] != -INFINITY)
          for (int t = 0; t < PS_ORIGIN_THREADS; ++t) {
            const double y = x[(size_t)h * PS_ORIGIN_THREADS + t];
            if (y != -INFINITY) bsum[h] += exp(y - bmax[h]);
          }
        const int64_t at = origin_partial_at(h, b, nblk);
        if (at < 0 || at + 1 >= (int64_t)part.size()) abort();
        part[(size_t)at] = bmax[h];
        part[(size_t)at + 1] = bsum[h];
      }
    });
    // brute force: move the field to the candidate, read it at the finding, in the order given
    int64_t bad = -1;
    long long nfinite = 0;
    for (int64_t i = 0; i < ncell && bad < 0; ++i) {
      const int r = (int)(i / N), c = (int)(i % N);
      for (int h = 0; h < nhyp; ++h) {
        bool dead = false;
        long double acc = 0.0L;
        for (int o = 0; o < nfind; ++o) {
          const int y = row[o] - (r - R), x = col[o] - (c - R);       // the finding in the moved field's frame
          const double v = (y >= 0 && y < N && x >= 0 && x < N) ? field[(size_t)y * N + x] : 0.0;
          const double t = origin_term(kind[o], (rate[o] * amount[h]) * v, cnt[o], lgamma(cnt[o] + 1.0));
          if (t == -INFINITY) dead = true;
          acc += t;
        }
        const double got = L[(size_t)h * ncell + i];
        if (dead != (got == -INFINITY)) bad = i;                      // the pattern: exact
        if (!dead && fabsl((long double)got - acc) > 1e-12L * (1.0L + fabsl(acc))) bad = i;
        if (!dead) {
          nfinite += 1;
          lse_ref[(size_t)h * ncell + i] += weights[member] * exp((double)acc);
        }
      }
    }
    if (bad >= 0) return fail("shifted read", N, bad / N, bad % N);
    if (nfinite == 0 || nfinite == (long long)nhyp * ncell) return fail("degenerate case", N, nfinite, 0);
    for (size_t k = 0; k < part.size(); ++k)
      if (isnan(part[k])) return fail("partial never written", N, (long long)k, 0);
    // stage two: one emulated wave per hypothesis, the lanes' chunks in index order, the lanes in lane order
    for (int h = 0; h < nhyp; ++h) {
      double mx = -INFINITY;
      for (int64_t b = 0; b < nblk; ++b) mx = fmax(mx, part[(size_t)origin_partial_at(h, b, nblk)]);
      double lanes[PS_ORIGIN_LANES], s = 0.0;
      int64_t covered = 0;
      for (int l = 0; l < PS_ORIGIN_LANES; ++l) {
        lanes[l] = mx == -INFINITY ? 0.0 : origin_lane_sum(part.data(), h, nblk, l, mx);
        const int64_t b0 = l * origin_chunk(nblk), b1 = b0 + origin_chunk(nblk) < nblk ? b0 + origin_chunk(nblk) : nblk;
        if (b1 > b0) covered += b1 - b0;
      }
      if (covered != nblk) return fail("chunks do not tile the partials", N, covered, nblk);
      for (int l = 0; l < PS_ORIGIN_LANES; ++l) s += lanes[l];
      long double direct = 0.0L;
      for (int64_t i = 0; i < ncell; ++i)
        if (L[(size_t)h * ncell + i] != -INFINITY) direct += expl((long double)L[(size_t)h * ncell + i] - mx);
      if (fabsl(direct - s) > 1e-12L * direct) return fail("row reduction", N, h, member);
    }
    *cases += 1;
  }
  // (A, S) against the direct sums, and the pattern of -inf
  for (size_t k = 0; k < A.size(); ++k) {
    const bool none = lse_ref[k] == 0.0;
    if (none != (A[k] == -INFINITY)) return fail("accumulated pattern", N, (long long)k, 0);
    if (!none && fabs(A[k] + log(S[k]) - log(lse_ref[k])) > 1e-11) return fail("accumulated value", N, (long long)k, 0);
  }
  return 0;
}

static int run_groups(int* cases) {
  for (int ng = 1; ng <= PS_ORIGIN_MAX_GROUP; ++ng) {
    int next = 0;
    for (int pass = 0; pass < 2; ++pass)
      for (int g = 0; g < ng; ++g) {
        for (int wrong = -1; wrong <= ng; ++wrong)
          if (wrong != g && origin_next_group(next, wrong, ng) != -1) return fail("group order accepts", ng, next, wrong);
        next = origin_next_group(next, g, ng);
        if (next != (g + 1) % ng) return fail("group order", ng, g, next);
      }
    *cases += 1;
  }
  // the streaming pair: -inf adds nothing, another order moves the value within rounding
  double a = -INFINITY, s = 0.0, a2 = -INFINITY, s2 = 0.0;
  const double x[5] = {-700.5, -3.25, -INFINITY, -1000.0, -3.0};
  for (int k = 0; k < 5; ++k) origin_lse_add(&a, &s, x[k], k + 1.0);
  for (int k = 4; k >= 0; --k) origin_lse_add(&a2, &s2, x[k], k + 1.0);
  if (a != -3.0 || a2 != -3.0 || fabs(a + log(s) - (a2 + log(s2))) > 1e-14) return fail("lse order", 0, 0, 0);
  double a3 = -INFINITY, s3 = 0.0;
  origin_lse_add(&a3, &s3, -INFINITY, 2.0);
  if (a3 != -INFINITY || s3 != 0.0) return fail("lse -inf", 0, 0, 0);
  *cases += 1;
  return 0;
}

int main(int argc, char** argv) {
  int cases = 0;
  if (run_groups(&cases)) return 1;
  for (int k = 1; k < argc; ++k)
    if (run_size(atoi(argv[k]), &cases)) return 1;
  printf("ok %d\n", cases);
  return 0;
}
