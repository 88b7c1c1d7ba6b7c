// Host emulation of the patch maps' device logic (parasitoids_amd/csrc/ps_patch_core.h): link, flatten, sizes and
// pick on crafted shapes, against a flood fill of its own.  Run 1: one thread, the cells in a scrambled order.
// Run 2: 8 std::threads joining concurrently through std::atomic<uint32_t>.  Every loop of the core is capped at
// 4 N N passes (Ops::step); a cap that is hit, a lost edge, or a wrong label, size, main patch or largest satellite
// fails the run.  Usage: patch_emul [N ...] (default 17 33); prints "ok <cases>" and exits 0, or the first failure.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "../../parasitoids_amd/csrc/ps_patch_core.h"

typedef std::vector<uint8_t> Mask;

struct Shape {
  std::string name;
  Mask m;
};

static std::vector<Shape> shapes(int N) {
  std::vector<Shape> out;
  auto blank = [&]() { return Mask((size_t)N * N, 0); };
  auto set = [&](Mask& m, int r, int c) { m[(size_t)r * N + c] = 1; };
  auto block = [&](Mask& m, int r0, int r1, int c0, int c1) {
    for (int r = r0; r <= r1; ++r)
      for (int c = c0; c <= c1; ++c) set(m, r, c);
  };
  Mask m = blank();
  out.push_back({"empty", m});
  out.push_back({"full", Mask((size_t)N * N, 1)});
  m = blank(), set(m, 0, 0), out.push_back({"first", m});
  m = blank(), set(m, N - 1, N - 1), out.push_back({"last", m});
  m = blank();
  for (int r = 0; r < N; ++r)
    for (int c = 0; c < N; ++c)
      if ((r + c) % 2 == 0) set(m, r, c);
  out.push_back({"checkerboard", m});
  {   // a one-cell-wide spiral: advance while the cell after the next is free, else turn right
    m = blank();
    const int dr[4] = {0, 1, 0, -1}, dc[4] = {1, 0, -1, 0};
    auto inb = [&](int r, int c) { return r >= 0 && r < N && c >= 0 && c < N; };
    int r = 0, c = 0, d = 0, turned = 0;
    set(m, 0, 0);
    while (turned < 2) {
      const int nr = r + dr[d], nc = c + dc[d], fr = nr + dr[d], fc = nc + dc[d];
      if (inb(nr, nc) && !m[(size_t)nr * N + nc] && !(inb(fr, fc) && m[(size_t)fr * N + fc])) {
        r = nr, c = nc, turned = 0;
        set(m, r, c);
      } else {
        d = (d + 1) % 4, ++turned;
      }
    }
    out.push_back({"spiral", m});
  }
  m = blank();
  for (int c = 0; c < N; c += 2) block(m, 0, N - 2, c, c);
  block(m, N - 1, N - 1, 0, N - 1);
  out.push_back({"comb", m});
  m = blank(), block(m, 1, 2, 1, 3), block(m, 5, 6, 8, 10), out.push_back({"equal_left_first", m});
  m = blank(), block(m, 1, 2, 8, 10), block(m, 5, 6, 1, 3), out.push_back({"equal_right_first", m});
  m = blank(), block(m, 2, 3, 2, 3), block(m, 4, 5, 4, 5), out.push_back({"diagonal", m});
  m = blank(), block(m, 2, 3, 6, 7), block(m, 4, 5, 4, 5), out.push_back({"antidiagonal", m});
  m = blank(), block(m, 2, 8, 2, 8);
  for (int r = 3; r <= 7; ++r)
    for (int c = 3; c <= 7; ++c) m[(size_t)r * N + c] = 0;
  set(m, 5, 5), out.push_back({"ring_island", m});
  m = blank(), set(m, 3, N - 1), set(m, 4, 0), out.push_back({"edge_next_row", m});
  m = blank(), set(m, 3, N - 1), set(m, 5, 0), out.push_back({"edge_two_rows", m});
  m = blank(), block(m, N - 1, N - 1, 0, N - 1), block(m, 0, N - 1, N - 1, N - 1), out.push_back({"last_row_col", m});
  return out;
}

// label[c] = the smallest index of c's component, PATCH_NONE outside the set: an explicit-stack flood fill
static std::vector<uint32_t> flood(const Mask& m, int N, int conn) {
  std::vector<uint32_t> lab((size_t)N * N, PATCH_NONE);
  std::vector<uint32_t> stack;
  for (uint32_t s = 0; s < (uint32_t)(N * N); ++s) {
    if (!m[s] || lab[s] != PATCH_NONE) continue;   // ascending s: the first cell met is the smallest
    lab[s] = s;
    stack.push_back(s);
    while (!stack.empty()) {
      const uint32_t c = stack.back();
      stack.pop_back();
      const int r = (int)(c / N), q = (int)(c % N);
      for (int dr = -1; dr <= 1; ++dr)
        for (int dc = -1; dc <= 1; ++dc) {
          if ((dr == 0 && dc == 0) || (conn == 4 && dr != 0 && dc != 0)) continue;
          const int rr = r + dr, cc = q + dc;
          if (rr < 0 || rr >= N || cc < 0 || cc >= N) continue;
          const uint32_t n = (uint32_t)(rr * N + cc);
          if (m[n] && lab[n] == PATCH_NONE) lab[n] = s, stack.push_back(n);
        }
    }
  }
  return lab;
}

static std::atomic<bool> g_capped{false};

template <class Word>
struct Ops {
  Word* parent;
  uint64_t cap, passes = 0;
  uint32_t load(uint32_t i);
  uint32_t cas(uint32_t i, uint32_t e, uint32_t d);
  bool step() {
    if (++passes <= cap) return true;
    g_capped = true;
    return false;
  }
};
template <>
uint32_t Ops<uint32_t>::load(uint32_t i) { return parent[i]; }
template <>
uint32_t Ops<uint32_t>::cas(uint32_t i, uint32_t e, uint32_t d) {
  const uint32_t old = parent[i];
  if (old == e) parent[i] = d;
  return old;
}
template <>
uint32_t Ops<std::atomic<uint32_t>>::load(uint32_t i) { return parent[i].load(std::memory_order_relaxed); }
template <>
uint32_t Ops<std::atomic<uint32_t>>::cas(uint32_t i, uint32_t e, uint32_t d) {
  parent[i].compare_exchange_strong(e, d, std::memory_order_relaxed);
  return e;   // the value found: e itself where the swap was made
}

// the cells in a scrambled order (Fisher-Yates with a 64-bit LCG)
static std::vector<uint32_t> scrambled(uint32_t n, uint64_t seed) {
  std::vector<uint32_t> o(n);
  for (uint32_t i = 0; i < n; ++i) o[i] = i;
  uint64_t x = seed * 2862933555777941757ull + 3037000493ull;
  for (uint32_t i = n; i > 1; --i) {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    std::swap(o[i - 1], o[(x >> 33) % i]);
  }
  return o;
}

template <class Word>
static void link_cells(Word* parent, const std::vector<uint32_t>& order, size_t first, size_t stride, int N, int conn) {
  for (size_t i = first; i < order.size(); i += stride) {
    Ops<Word> at{parent, 4ull * N * N};   // the cap holds per cell: every loop under it stays below
    const uint32_t c = order[i];
    if (at.load(c) == PATCH_NONE) continue;
    patch_link_cell(at, c, (uint32_t)N, conn);
  }
}

// flatten, sizes, pick and the second maximum as the kernels do them, checked against the flood fill
template <class Word>
static bool check(Word* parent, const std::vector<uint32_t>& want, int N, const char* what) {
  const uint32_t n = (uint32_t)(N * N);
  std::vector<uint32_t> root(n, PATCH_NONE), size(n, 0), wsize(n, 0);
  for (uint32_t c = 0; c < n; ++c) {
    Ops<Word> at{parent, 4ull * N * N};
    if (at.load(c) != PATCH_NONE) root[c] = patch_find(at, c);
    if (root[c] != want[c]) {
      printf("FAIL %s: cell %u has root %u, the flood fill %u\n", what, c, root[c], want[c]);
      return false;
    }
    if (want[c] != PATCH_NONE) ++size[root[c]], ++wsize[want[c]];
  }
  uint64_t key = 0;
  uint32_t wcells = 0, wlabel = PATCH_NONE;
  for (uint32_t c = 0; c < n; ++c) {
    if (root[c] == c) key = std::max(key, patch_key(size[c], c));
    if (want[c] == c && wsize[c] > wcells) wcells = wsize[c], wlabel = c;   // ascending c: among equals the first stays
  }
  const uint32_t label = patch_key_label(key);
  if (patch_key_cells(key) != wcells || label != wlabel) {
    printf("FAIL %s: main patch (%u cells, label %u), wanted (%u, %u)\n", what, patch_key_cells(key), label, wcells, wlabel);
    return false;
  }
  uint32_t sat = 0, wsat = 0;
  for (uint32_t c = 0; c < n; ++c) {
    if (root[c] == c && c != label) sat = std::max(sat, size[c]);
    if (want[c] == c && c != wlabel) wsat = std::max(wsat, wsize[c]);
  }
  if (sat != wsat) {
    printf("FAIL %s: largest satellite %u, wanted %u\n", what, sat, wsat);
    return false;
  }
  return true;
}

int main(int argc, char** argv) {
  std::vector<int> sizes;
  for (int i = 1; i < argc; ++i) sizes.push_back(atoi(argv[i]));
  if (sizes.empty()) sizes = {17, 33};
  int cases = 0;
  for (int N : sizes) {
    if (N < 12) {
      printf("FAIL: the shapes need N >= 12\n");
      return 2;
    }
    const uint32_t n = (uint32_t)(N * N);
    for (const Shape& sh : shapes(N))
      for (int conn : {4, 8}) {
        const std::vector<uint32_t> want = flood(sh.m, N, conn);
        char what[128];
        for (uint64_t seed = 1; seed <= 3; ++seed) {
          const std::vector<uint32_t> order = scrambled(n, seed * 977 + (uint64_t)N);
          // run 1: thread by thread
          std::vector<uint32_t> p1(n);
          for (uint32_t c = 0; c < n; ++c) p1[c] = sh.m[c] ? c : PATCH_NONE;
          link_cells(p1.data(), order, 0, 1, N, conn);
          snprintf(what, sizeof what, "%s N=%d conn=%d seed=%d serial", sh.name.c_str(), N, conn, (int)seed);
          if (g_capped || !check(p1.data(), want, N, what)) {
            if (g_capped) printf("FAIL %s: a loop ran past 4 N N passes\n", what);
            return 1;
          }
          // run 2: 8 threads, each a strided share of the scrambled order, joining concurrently
          std::vector<std::atomic<uint32_t>> p2(n);
          for (uint32_t c = 0; c < n; ++c) p2[c].store(sh.m[c] ? c : PATCH_NONE, std::memory_order_relaxed);
          std::vector<std::thread> th;
          for (int t = 0; t < 8; ++t)
            th.emplace_back([&, t]() { link_cells(p2.data(), order, (size_t)t, 8, N, conn); });
          for (auto& t : th) t.join();
          snprintf(what, sizeof what, "%s N=%d conn=%d seed=%d threads", sh.name.c_str(), N, conn, (int)seed);
          if (g_capped || !check(p2.data(), want, N, what)) {
            if (g_capped) printf("FAIL %s: a loop ran past 4 N N passes\n", what);
            return 1;
          }
          cases += 2;
        }
      }
  }
  printf("ok %d\n", cases);
  return 0;
}
