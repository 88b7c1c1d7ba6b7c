// Host emulation of the origin maps' known-release logic (csrc/ps_origin_core.h): the background read of every
// finding for every known release -- at the centre, at the far corners of the offset range, off the domain on one
// axis only -- against a brute force that moves the field to the release and reads it at the finding; the terms
// summed in index order across the known groups by the last group's pass, as the device does; the null row in the
// kernel's order q; the identity l_h(s) == l0 at a candidate whose shifted reads are all 0; and the order of one
// member's calls: the known groups 0 .. nk - 1, then the adds.  The lanes of one emulated launch run on 8 threads.
// Prints "ok <cases>" or "FAIL ..." and exits 1.
//   origin_known_emul N [N ...]
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

// positive everywhere but a band of exact zeros: a read that lands in the domain is told from one that does not
static std::vector<double> make_field(int N, int which) {
  std::vector<double> f((size_t)N * N, 0.0);
  for (int y = 0; y < N; ++y)
    for (int x = 0; x < N; ++x)
      if ((x + 2 * y + which) % 11 != 0) f[(size_t)y * N + x] = 0.25 + 0.001 * ((7 * y + 3 * x + which) % 97);
  return f;
}

static int run_size(int N, int* cases) {
  const int R = N / 2, nfind = 9, nknown = 6, nk = 2;
  // findings: the four corners, the centre, and four more; every kind, a count of 0 among them
  const int32_t row[nfind] = {0, 0, N - 1, N - 1, R, R - R / 4, R + R / 3, 1, N - 2};
  const int32_t col[nfind] = {0, N - 1, 0, N - 1, R, R + R / 3, R + R / 4, N - 2, 1};
  const int32_t kind[nfind] = {PS_ORIGIN_NONE, PS_ORIGIN_COUNT, PS_ORIGIN_NONE, PS_ORIGIN_FOUND, PS_ORIGIN_COUNT,
                               PS_ORIGIN_COUNT, PS_ORIGIN_FOUND, PS_ORIGIN_COUNT, PS_ORIGIN_NONE};
  const double cnt[nfind] = {0, 0, 0, 0, 3, 1, 0, 2, 0};
  const double rate[nfind] = {0.5, 0.25, 1.0, 0.125, 0.5, 2.0, 0.75, 0.3, 0.7};
  // known releases: the centre; the four extremes of the offset range; one that leaves on the row axis only for the
  // findings of the last rows.  Groups interleaved, so the sum in index order crosses the groups.
  const int32_t drow[nknown] = {0, N - 1, -(N - 1), 3, R + 1, -2};
  const int32_t dcol[nknown] = {0, -(N - 1), N - 1, -5, 0, R};
  const double amount[nknown] = {1.0, 0.3, 0.7, 2.0, 0.125, 1.5};
  const int32_t kgroup[nknown] = {0, 1, 0, 1, 0, 1};
  int32_t order[nfind];
  origin_order(nfind, kind, cnt, order);
  std::vector<OriginFinding> find(nfind);
  std::vector<double> rak((size_t)nknown * nfind);
  for (int q = 0; q < nfind; ++q) {
    const int o = order[q];
    find[q] = OriginFinding{row[o] + R, col[o] + R, 0, kind[o], cnt[o], lgamma(cnt[o] + 1.0)};
    for (int k = 0; k < nknown; ++k) rak[(size_t)k * nfind + q] = rate[o] * amount[k];
  }
  const std::vector<double> field[nk] = {make_field(N, 0), make_field(N, 1)};   // one record per known group
  std::vector<double> term((size_t)nknown * nfind, NAN), bg(nfind, NAN), lterm(nfind, NAN);
  // the launches: one per known group, lane q owns finding q and walks the group's releases in index order; the
  // last group's launch also forms bg and the terms at bg
  for (int g = 0; g < nk; ++g) {
    const bool last = g + 1 == nk;
    on_threads(nfind, [&](int64_t q) {
      for (int k = 0; k < nknown; ++k) {
        if (kgroup[k] != g) continue;
        int64_t src;
        double v = 0.0;
        if (origin_known_source(N, find[q].rowR, find[q].colR, drow[k], dcol[k], &src))
          v = field[g][(size_t)src];                                     // ASan watches src
        const size_t at = (size_t)k * nfind + q;
        if (at >= term.size()) abort();
        term[at] = origin_bg_term(rak[at], v);
      }
      if (last) {
        bg[q] = origin_bg_sum(term.data(), nknown, nfind, (int)q);
        lterm[q] = origin_term(find[q].kind, bg[q], find[q].n, find[q].lgam);
      }
    });
  }
  const double l0 = origin_null_sum(lterm.data(), nfind);
  // brute force: the field moved to the release, read at the finding; per axis, never by the flat index
  int inside = 0, outside = 0, one_axis = 0;
  for (int q = 0; q < nfind; ++q) {
    const int o = order[q];
    double s = 0.0;
    for (int k = 0; k < nknown; ++k) {
      const int y = row[o] - drow[k], x = col[o] - dcol[k];
      const bool yin = y >= 0 && y < N, xin = x >= 0 && x < N;
      const double v = yin && xin ? field[kgroup[k]][(size_t)y * N + x] : 0.0;
      inside += yin && xin;
      outside += !(yin && xin);
      one_axis += yin != xin;
      const double t = (rate[o] * amount[k]) * v;
      if (!same_bits(t, term[(size_t)k * nfind + q])) return fail("background term", N, q, k);
      s = s + t;
    }
    if (!same_bits(s, bg[q])) return fail("background sum", N, q, 0);
  }
  if (inside == 0 || outside == 0 || one_axis == 0) return fail("degenerate offsets", N, inside, one_axis);
  // the null row: the kernel's order q, from +0.0
  double want = 0.0;
  for (int q = 0; q < nfind; ++q) want = want + origin_term(find[q].kind, bg[q], find[q].n, find[q].lgam);
  if (!same_bits(want, l0)) return fail("null row order", N, 0, 0);
  // the identity: a candidate whose shifted reads are all 0 ends at l0, bit for bit, under every amount
  const double amounts[3] = {0.25, 0.5, 1.0};
  for (int h = 0; h < 3; ++h) {
    double acc = 0.0;
    for (int q = 0; q < nfind; ++q) {
      const double mu = origin_mu_bg(bg[q], rate[order[q]] * amounts[h], 0.0);
      acc = acc + origin_term(find[q].kind, mu, find[q].n, find[q].lgam);
    }
    if (!same_bits(acc, l0)) return fail("identity", N, h, 0);
  }
  // a finding excludes a cell only where bg == 0 and v == 0
  if (origin_term(PS_ORIGIN_FOUND, origin_mu_bg(0.0, 2.0, 0.0), 0.0, 0.0) != -INFINITY ||
      origin_term(PS_ORIGIN_FOUND, origin_mu_bg(0.5, 2.0, 0.0), 0.0, 0.0) == -INFINITY ||
      origin_term(PS_ORIGIN_FOUND, origin_mu_bg(0.0, 2.0, 0.5), 0.0, 0.0) == -INFINITY)
    return fail("exclusion", N, 0, 0);
  *cases += 1;
  return 0;
}

// one member: backgrounds 0 .. nk - 1 in order, then the adds 0 .. ng - 1; everything else is refused
static int run_protocol(int* cases) {
  for (int nk = 1; nk <= PS_ORIGIN_MAX_KGROUP; ++nk)
    for (int ng = 1; ng <= PS_ORIGIN_MAX_GROUP; ++ng) {
      int next_bg = 0, next_group = 0;
      for (int member = 0; member < 2; ++member) {
        for (int g = 0; g < nk; ++g) {
          if (origin_backgrounds_done(next_bg, nk)) return fail("adds allowed early", nk, ng, g);
          for (int wrong = -1; wrong <= nk; ++wrong)
            if (wrong != g && origin_next_background(next_bg, next_group, wrong, nk) != -1)
              return fail("background order accepts", nk, next_bg, wrong);
          next_bg = origin_next_background(next_bg, next_group, g, nk);
          if (next_bg != g + 1) return fail("background order", nk, g, next_bg);
        }
        if (!origin_backgrounds_done(next_bg, nk)) return fail("backgrounds not done", nk, ng, next_bg);
        for (int g = 0; g < ng; ++g) {
          for (int k = 0; k < nk; ++k)   // complete: no further background, and none while the adds are under way
            if (origin_next_background(next_bg, next_group, k, nk) != -1)
              return fail("background after the backgrounds", nk, g, k);
          next_group = origin_next_group(next_group, g, ng);
          if (next_group != (g + 1) % ng) return fail("group order", ng, g, next_group);
        }
        next_bg = 0;   // the member is in
      }
      *cases += 1;
    }
  if (!origin_backgrounds_done(0, 0)) return fail("a handle without known releases", 0, 0, 0);
  return 0;
}

int main(int argc, char** argv) {
  int cases = 0;
  if (run_protocol(&cases)) return 1;
  for (int k = 1; k < argc; ++k)
    if (run_size(atoi(argv[k]), &cases)) return 1;
  printf("ok %d\n", cases);
  return 0;
}
