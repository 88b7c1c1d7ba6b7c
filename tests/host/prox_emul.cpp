// Host emulation of the proximity fields' device logic (csrc/ps_prox_core.h): the set as 64-bit words in the flat
// layout of the device (bit c & 63 of word c >> 6, c = y N + x), the row pass cell by cell, the column pass strip by
// strip with the strip's g staged as the kernel stages it, on 8 threads that each own whole cells -- against a brute
// force that knows neither pass.  Both sides, the crafted sets of tests/prox_ref.py and pseudo-random masks of three
// densities, every strip width from 64 down to 1.  Prints "ok <cases>" or "FAIL ..." and exits 1.
//   prox_emul N [N ...]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../parasitoids_amd/csrc/ps_prox_core.h"

typedef std::vector<uint8_t> Set;   // [N * N], 1 in the set

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

// the nearest cell of the set by rings of growing Chebyshev radius (dense sets) or over the list of its cells
static std::vector<uint32_t> brute(const Set& s, int N) {
  std::vector<std::pair<int, int>> cells;
  for (int y = 0; y < N; ++y)
    for (int x = 0; x < N; ++x)
      if (s[(size_t)y * N + x]) cells.push_back({y, x});
  std::vector<uint32_t> out((size_t)N * N, prox_far2(N));
  const bool sparse = cells.size() < 256;
  on_threads((int64_t)N * N, [&, sparse](int64_t c) {
    const int y = (int)(c / N), x = (int)(c % N);
    uint32_t best = prox_far2(N);
    if (sparse) {
      for (auto& p : cells) {
        const uint32_t d = (uint32_t)((y - p.first) * (y - p.first) + (x - p.second) * (x - p.second));
        if (d < best) best = d;
      }
    } else {
      for (int r = 0; r < N && (uint32_t)r * r < best; ++r)
        for (int yy = y - r; yy <= y + r; ++yy) {
          if (yy < 0 || yy >= N) continue;
          const bool edge = yy == y - r || yy == y + r;
          for (int xx = x - r; xx <= x + r; xx += edge ? 1 : 2 * r > 0 ? 2 * r : 1) {
            if (xx < 0 || xx >= N || !s[(size_t)yy * N + xx]) continue;
            const uint32_t d = (uint32_t)((y - yy) * (y - yy) + (x - xx) * (x - xx));
            if (d < best) best = d;
          }
        }
    }
    out[(size_t)c] = best;
  });
  return out;
}

// both passes as the device runs them, the column pass over strips of W columns
static std::vector<uint32_t> two_pass(const Set& s, int N, int W) {
  const int64_t ncell = (int64_t)N * N, pitch = (ncell + 63) / 64 * 64;
  std::vector<uint64_t> words((size_t)(pitch >> 6), 0);
  on_threads(pitch >> 6, [&](int64_t w) {   // a wave's ballot
    uint64_t m = 0;
    for (int b = 0; b < 64; ++b) {
      const int64_t c = w * 64 + b;
      if (c < ncell && s[(size_t)c]) m |= 1ull << b;
    }
    words[(size_t)w] = m;
  });
  std::vector<uint16_t> g((size_t)ncell);
  on_threads(ncell, [&](int64_t c) {
    const int64_t lo = c / N * N;
    g[(size_t)c] = (uint16_t)prox_row_dist(words.data(), lo, lo + N - 1, c);
  });
  std::vector<uint32_t> out((size_t)ncell);
  const uint32_t far2 = prox_far2(N);
  const int nstrip = (N + W - 1) / W;
  std::vector<uint16_t> lds((size_t)nstrip * N * W);   // every workgroup's staged strip, [strip][N][W]
  for (int k = 0; k < nstrip; ++k)
    for (int y = 0; y < N; ++y)
      for (int lx = 0; lx < W; ++lx)
        lds[((size_t)k * N + y) * W + lx] = k * W + lx < N ? g[(size_t)y * N + k * W + lx] : (uint16_t)PROX_NONE;
  on_threads((int64_t)nstrip * N * W, [&](int64_t i) {
    const int k = (int)(i / ((int64_t)N * W)), y = (int)(i / W % N), lx = (int)(i % W);
    if (k * W + lx < N)
      out[(size_t)y * N + k * W + lx] = prox_col_search(lds.data() + (size_t)k * N * W + lx, W, y, N, far2);
  });
  return out;
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (double)(rng_state >> 11) / 9007199254740992.0;
}

static std::vector<std::pair<std::string, Set>> cases(int N) {
  std::vector<std::pair<std::string, Set>> out;
  auto blank = [&] { return Set((size_t)N * N, 0); };
  auto at = [&](Set& s, int y, int x) -> uint8_t& { return s[(size_t)y * N + x]; };
  const int c = N / 2;
  const int corner[4][2] = {{0, 0}, {0, N - 1}, {N - 1, 0}, {N - 1, N - 1}};
  for (int k = 0; k < 4; ++k) {
    Set s = blank();
    at(s, corner[k][0], corner[k][1]) = 1;
    out.push_back({"corner" + std::to_string(k), s});
  }
  { Set s = blank(); at(s, c, c) = 1; out.push_back({"centre", s}); }
  { Set s = blank(); for (int x = 0; x < N; ++x) at(s, c / 2, x) = 1; out.push_back({"row", s}); }
  { Set s = blank(); for (int y = 0; y < N; ++y) at(s, y, c / 2) = 1; out.push_back({"column", s}); }
  for (int col : {63, 64, N - 1}) {
    if (col >= N) continue;
    Set s = blank();
    for (int y = 0; y < N; ++y) at(s, y, col) = 1;
    out.push_back({"column" + std::to_string(col), s});
  }
  { Set s = blank(); at(s, c, c - 5) = 1; at(s, c, c + 5) = 1; out.push_back({"equidistant", s}); }
  { Set s = blank(); for (int y = 0; y < N; ++y) for (int x = 0; x < N; ++x) at(s, y, x) = (y + x) & 1; out.push_back({"checkerboard", s}); }
  {
    Set s = blank();
    for (int y = 0; y < N; ++y)
      for (int x = 0; x < N; ++x) {
        const int d = (y - c) * (y - c) + (x - c) * (x - c);
        at(s, y, x) = d >= (N / 8) * (N / 8) && d <= (N / 3) * (N / 3);
      }
    out.push_back({"ring", s});
  }
  out.push_back({"empty", blank()});
  out.push_back({"whole", Set((size_t)N * N, 1)});
  for (double p : {0.002, 0.05, 0.6}) {
    Set s = blank();
    for (auto& v : s) v = rnd() < p;
    out.push_back({"random" + std::to_string(p), s});
  }
  return out;
}

int main(int argc, char** argv) {
  long ncase = 0;
  for (int a = 1; a < argc; ++a) {
    const int N = atoi(argv[a]);
    if (N < 1 || N > PROX_MAX_N) {
      printf("FAIL size %s\n", argv[a]);
      return 1;
    }
    if (prox_strip_width(801, 160 * 1024) != 64 || prox_strip_width(1281, 160 * 1024) != 32 ||
        prox_strip_width(4097, 160 * 1024) != 16 || prox_strip_width(32767, 160 * 1024) != 2) {
      printf("FAIL strip width\n");
      return 1;
    }
    for (auto& kv : cases(N))
      for (int side = 0; side < 2; ++side) {
        Set s = kv.second;
        if (side)
          for (auto& v : s) v = !v;
        const std::vector<uint32_t> want = brute(s, N);
        for (int W = 64; W >= 1; W >>= 1) {
          const std::vector<uint32_t> got = two_pass(s, N, W);
          for (size_t i = 0; i < want.size(); ++i)
            if (got[i] != want[i]) {
              printf("FAIL N %d %s side %d strip %d cell (%d, %d): %u, brute force %u\n", N, kv.first.c_str(), side, W,
                     (int)(i / N), (int)(i % N), got[i], want[i]);
              return 1;
            }
        }
        ++ncase;
      }
  }
  printf("ok %ld\n", ncase);
  return 0;
}
