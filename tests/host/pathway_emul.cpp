// Host emulation of the pathway maps' device logic (parasitoids_amd/csrc/ps_pathway_core.h over the labelling of
// ps_patch_core.h): per slot link, flatten, flag and class, thread by thread, on time sequences of masks -- crafted
// ones and pseudo-random blobs that appear, grow, vanish and merge -- against a flood fill and a patch-by-patch
// classification of its own.  Run 1: one thread, the cells of every pass in a scrambled order.  Run 2: 8 std::threads
// through std::atomic<uint32_t>, a join between the passes where the device has a launch boundary.  Every loop of the
// labelling is capped at 4 N N passes (Ops::step); a cap that is hit, or a wrong state, row or focus count fails the
// run.  Usage: pathway_emul [N ...] (default 17 33 65); prints "ok <cases>" and exits 0, or the first failure.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "../../parasitoids_amd/csrc/ps_patch_core.h"
#include "../../parasitoids_amd/csrc/ps_pathway_core.h"

typedef std::vector<uint8_t> Mask;
static const int NSLOT = 5;

struct Seq {
  std::string name;
  std::vector<Mask> m;            // [NSLOT] masks
  std::vector<uint32_t> anchors;  // linear indices
};

static uint64_t lcg(uint64_t& x) {
  x = x * 6364136223846793005ull + 1442695040888963407ull;
  return x >> 33;
}

static std::vector<Seq> sequences(int N) {
  std::vector<Seq> out;
  const int c = N / 2;
  const uint32_t centre = (uint32_t)(c * N + c);
  auto blank = [&]() { return std::vector<Mask>(NSLOT, Mask((size_t)N * N, 0)); };
  auto block = [&](std::vector<Mask>& m, int s0, int s1, int r0, int r1, int c0, int c1, uint8_t v) {
    for (int s = s0; s <= s1; ++s)
      for (int r = std::max(r0, 0); r <= std::min(r1, N - 1); ++r)
        for (int q = std::max(c0, 0); q <= std::min(c1, N - 1); ++q) m[(size_t)s][(size_t)r * N + q] = v;
  };
  auto origin = [&](std::vector<Mask>& m) { block(m, 0, NSLOT - 1, c - 1, c + 1, c - 1, c + 1, 1); };
  std::vector<Mask> m = blank();
  out.push_back({"empty", m, {centre}});
  m = blank();
  for (int s = 0; s < NSLOT; ++s) block(m, s, s, c - s - 1, c + s + 1, c - s - 1, c + s + 1, 1);
  out.push_back({"grow", m, {centre}});
  m = blank(), origin(m);
  block(m, 0, NSLOT - 1, c - 1, c + 1, c + 5, c + 6, 1);   // jump
  block(m, 1, NSLOT - 1, c - 1, c + 1, c + 4, c + 7, 1);   // secondary
  block(m, 2, NSLOT - 1, c, c, c + 2, c + 3, 1);           // the bridge: front from here on
  block(m, 3, NSLOT - 1, c - 2, c + 2, c + 8, c + 8, 1);
  out.push_back({"jump_grow_merge", m, {centre}});
  m = blank(), origin(m);
  block(m, 1, NSLOT - 1, c + 2, c + 3, c + 2, c + 3, 1);   // diagonal to the origin
  block(m, 1, NSLOT - 1, c - 6, c - 5, c - 6, c - 5, 1);
  out.push_back({"two_foci_diagonal", m, {centre}});
  m = blank(), origin(m);
  block(m, 0, 0, c + 4, c + 5, c - 6, c - 4, 1);           // a focus that drops out ...
  block(m, 2, 2, c + 5, c + 7, c - 4, c - 3, 1);           // ... and whose ground is re-entered
  block(m, 4, 4, 1, 2, 1, 2, 1);
  out.push_back({"dropout_reenter", m, {centre}});
  m = blank();
  block(m, 0, NSLOT - 1, 2, 3, 2, 4, 1);
  for (int s = 1; s < NSLOT; ++s) block(m, s, s, c - s, c + s, c - s, c + s, 1);
  out.push_back({"anchor_late", m, {centre}});
  m = blank(), origin(m);
  block(m, 0, NSLOT - 1, 2, 4, 2, 4, 1);
  block(m, 1, NSLOT - 1, 2, 4, N - 5, N - 3, 1);
  out.push_back({"two_anchors", m, {centre, (uint32_t)(3 * N + 3)}});
  m = blank();
  block(m, 0, NSLOT - 1, c, c + 8, c, c + 8, 1);
  block(m, 0, NSLOT - 1, c + 1, c + 7, c + 1, c + 7, 0);   // the ring, a corner on the anchor
  block(m, 1, NSLOT - 1, c + 4, c + 4, c + 4, c + 4, 1);
  block(m, 2, NSLOT - 1, c + 3, c + 5, c + 4, c + 4, 1);
  block(m, 3, NSLOT - 1, c + 1, c + 3, c + 4, c + 4, 1);
  out.push_back({"ring_island", m, {centre}});
  m = blank(), origin(m);
  block(m, 1, NSLOT - 1, 3, 3, N - 1, N - 1, 1), block(m, 1, NSLOT - 1, 4, 4, 0, 0, 1);   // no wrap
  block(m, 2, NSLOT - 1, 3, 3, N - 2, N - 2, 1), block(m, 2, NSLOT - 1, 4, 4, 1, 1, 1);
  out.push_back({"edge_next_row", m, {centre}});
  m = blank(), origin(m);
  block(m, 2, NSLOT - 1, N - 1, N - 1, N - 1, N - 1, 1);
  out.push_back({"last", m, {centre}});
  // pseudo-random blobs: each lives over a span of slots and grows by one cell per slot; speckle on top
  for (int t = 0; t < 6; ++t) {
    uint64_t x = 88172645463325252ull + 7919ull * (uint64_t)t + (uint64_t)N;
    m = blank();
    const int nblob = 4 + N / 8;
    for (int b = 0; b < nblob; ++b) {
      const int r = (int)(lcg(x) % (uint64_t)N), q = (int)(lcg(x) % (uint64_t)N), h = (int)(lcg(x) % 3);
      const int s0 = (int)(lcg(x) % NSLOT), s1 = std::min(NSLOT - 1, s0 + (int)(lcg(x) % NSLOT));
      for (int s = s0; s <= s1; ++s) block(m, s, s, r - h - (s - s0), r + h + (s - s0), q - h, q + h + (s - s0), 1);
    }
    for (int s = 0; s < NSLOT; ++s)
      for (int i = 0; i < N; ++i) m[(size_t)s][(size_t)(lcg(x) % (uint64_t)(N * N))] = 1;
    if (t % 2 == 0) origin(m);
    std::vector<uint32_t> anchors = {centre};
    for (int a = 0; a < t; ++a) anchors.push_back((uint32_t)(lcg(x) % (uint64_t)(N * N)));
    out.push_back({"random" + std::to_string(t), m, anchors});
  }
  return out;
}

// label[c] = the smallest index of c's component, PATCH_NONE outside the set: an explicit-stack flood fill
static std::vector<uint32_t> flood(const Mask& m, int N, int conn) {
  std::vector<uint32_t> lab((size_t)N * N, PATCH_NONE);
  std::vector<uint32_t> stack;
  for (uint32_t s = 0; s < (uint32_t)(N * N); ++s) {
    if (!m[s] || lab[s] != PATCH_NONE) continue;
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

struct Result {
  std::vector<uint8_t> state;    // [N * N]
  std::vector<uint32_t> rows;    // [NSLOT][4]
};

// the definition, patch by patch: origin, seeded, then the class of the cells still unreached
static Result reference(const Seq& q, int N, int conn) {
  const uint32_t n = (uint32_t)(N * N);
  Result R{std::vector<uint8_t>(n, 0), std::vector<uint32_t>((size_t)NSLOT * 4, 0)};
  for (int s = 0; s < NSLOT; ++s) {
    const std::vector<uint32_t> lab = flood(q.m[(size_t)s], N, conn);
    const std::vector<uint8_t> before = R.state;
    std::vector<uint8_t> origin(n, 0), seeded(n, 0);
    for (uint32_t c = 0; c < n; ++c) {
      if (lab[c] == PATCH_NONE) continue;
      if (before[c] == 1) origin[lab[c]] = 1;
      if (before[c] != 0) seeded[lab[c]] = 1;
    }
    for (uint32_t a : q.anchors)
      if (lab[a] != PATCH_NONE) origin[lab[a]] = 1;
    for (uint32_t c = 0; c < n; ++c) {
      if (lab[c] == PATCH_NONE) continue;
      const uint32_t l = lab[c];
      const uint8_t cls = origin[l] ? 1 : (seeded[l] ? 3 : 2);
      if (before[c] == 0) R.state[c] = cls, ++R.rows[(size_t)s * 4 + (cls - 1)];
      if (l == c && cls == 2) ++R.rows[(size_t)s * 4 + 3];
    }
  }
  return R;
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

static void word_or(uint32_t& w, uint32_t bits) { w |= bits; }
static void word_or(std::atomic<uint32_t>& w, uint32_t bits) { w.fetch_or(bits, std::memory_order_relaxed); }
static void word_add(uint32_t& w, uint32_t v) { w += v; }
static void word_add(std::atomic<uint32_t>& w, uint32_t v) { w.fetch_add(v, std::memory_order_relaxed); }
static uint32_t word_get(const uint32_t& w) { return w; }
static uint32_t word_get(const std::atomic<uint32_t>& w) { return w.load(std::memory_order_relaxed); }
static void word_set(uint32_t& w, uint32_t v) { w = v; }
static void word_set(std::atomic<uint32_t>& w, uint32_t v) { w.store(v, std::memory_order_relaxed); }

// the cells in a scrambled order (Fisher-Yates with a 64-bit LCG)
static std::vector<uint32_t> scrambled(uint32_t n, uint64_t seed) {
  std::vector<uint32_t> o(n);
  for (uint32_t i = 0; i < n; ++i) o[i] = i;
  uint64_t x = seed * 2862933555777941757ull + 3037000493ull;
  for (uint32_t i = n; i > 1; --i) std::swap(o[i - 1], o[lcg(x) % i]);
  return o;
}

// One slot's passes as the device runs them, each over the share (first, stride) of the scrambled cells.  The
// caller puts a join between two passes: that is the launch boundary.
template <class Word>
struct Slot {
  Word* parent;            // [n] the slot's labelling
  Word* flags;             // [n]
  uint8_t* state;          // [n] one writer per cell
  Word* row;               // [4]
  const std::vector<uint32_t>* order;
  const std::vector<uint32_t>* anchors;
  int N, conn;
  void link(size_t first, size_t stride) const {
    for (size_t i = first; i < order->size(); i += stride) {
      Ops<Word> at{parent, 4ull * N * N};   // the cap holds per cell: every loop under it stays below
      const uint32_t c = (*order)[i];
      if (at.load(c) == PATCH_NONE) continue;
      patch_link_cell(at, c, (uint32_t)N, conn);
    }
  }
  void flatten(size_t first, size_t stride) const {
    for (size_t i = first; i < order->size(); i += stride) {
      Ops<Word> at{parent, 4ull * N * N};
      const uint32_t c = (*order)[i];
      if (at.load(c) == PATCH_NONE) continue;
      word_set(parent[c], patch_find(at, c));   // an ancestor in place of an ancestor
    }
  }
  void flag(size_t first, size_t stride) const {
    for (size_t i = first; i < order->size(); i += stride) {
      const uint32_t c = (*order)[i], root = word_get(parent[c]);
      if (root == PATCH_NONE) continue;
      const uint32_t bits = pathway_flag_bits(state[c]);
      if (bits) word_or(flags[root], bits);
    }
    for (size_t a = first; a < anchors->size(); a += stride) {
      const uint32_t root = word_get(parent[(*anchors)[a]]);
      if (root != PATCH_NONE) word_or(flags[root], PATHWAY_ORIGIN);
    }
  }
  void classify(size_t first, size_t stride) const {
    for (size_t i = first; i < order->size(); i += stride) {
      const uint32_t c = (*order)[i], root = word_get(parent[c]);
      if (root == PATCH_NONE || state[c] != PATHWAY_UNREACHED) continue;
      const uint32_t f = word_get(flags[root]), cls = pathway_class(f);
      state[c] = (uint8_t)cls;
      word_add(row[cls - 1], 1);
      if (pathway_founds(c, root, f)) word_add(row[3], 1);
    }
  }
};

template <class Word>
static Result run(const Seq& q, int N, int conn, uint64_t seed, int nthread) {
  const uint32_t n = (uint32_t)(N * N);
  Result R{std::vector<uint8_t>(n, 0), std::vector<uint32_t>((size_t)NSLOT * 4, 0)};
  for (int s = 0; s < NSLOT; ++s) {
    std::vector<Word> parent(n), flags(n), row(4);
    for (uint32_t c = 0; c < n; ++c) word_set(parent[c], q.m[(size_t)s][c] ? c : PATCH_NONE), word_set(flags[c], 0);
    for (int f = 0; f < 4; ++f) word_set(row[(size_t)f], 0);
    const std::vector<uint32_t> order = scrambled(n, seed * 131 + (uint64_t)s);
    const Slot<Word> sl{parent.data(), flags.data(), R.state.data(), row.data(), &order, &q.anchors, N, conn};
    void (Slot<Word>::*passes[4])(size_t, size_t) const = {&Slot<Word>::link, &Slot<Word>::flatten, &Slot<Word>::flag,
                                                            &Slot<Word>::classify};
    for (auto pass : passes) {
      if (nthread == 1) {
        (sl.*pass)(0, 1);
      } else {
        std::vector<std::thread> th;
        for (int t = 0; t < nthread; ++t) th.emplace_back([&, t]() { (sl.*pass)((size_t)t, (size_t)nthread); });
        for (auto& t : th) t.join();
      }
    }
    for (int f = 0; f < 4; ++f) R.rows[(size_t)s * 4 + f] = word_get(row[(size_t)f]);
  }
  return R;
}

static bool same(const Result& got, const Result& want, const char* what) {
  for (size_t c = 0; c < want.state.size(); ++c)
    if (got.state[c] != want.state[c]) {
      printf("FAIL %s: cell %zu has state %d, the definition %d\n", what, c, got.state[c], want.state[c]);
      return false;
    }
  for (size_t i = 0; i < want.rows.size(); ++i)
    if (got.rows[i] != want.rows[i]) {
      printf("FAIL %s: slot %zu word %zu is %u, the definition %u\n", what, i / 4, i % 4, got.rows[i], want.rows[i]);
      return false;
    }
  return true;
}

int main(int argc, char** argv) {
  std::vector<int> sizes;
  for (int i = 1; i < argc; ++i) sizes.push_back(atoi(argv[i]));
  if (sizes.empty()) sizes = {17, 33, 65};
  int cases = 0;
  uint32_t seen[4] = {0, 0, 0, 0};
  for (int N : sizes) {
    if (N < 17 || N % 2 == 0) {
      printf("FAIL: the sequences need an odd N >= 17\n");
      return 2;
    }
    for (const Seq& q : sequences(N))
      for (int conn : {4, 8}) {
        const Result want = reference(q, N, conn);
        for (int s = 0; s < NSLOT; ++s)
          for (int f = 0; f < 4; ++f) seen[f] += want.rows[(size_t)s * 4 + f];
        char what[160];
        for (uint64_t seed = 1; seed <= 2; ++seed) {
          snprintf(what, sizeof what, "%s N=%d conn=%d seed=%d serial", q.name.c_str(), N, conn, (int)seed);
          const Result one = run<uint32_t>(q, N, conn, seed * 977 + (uint64_t)N, 1);
          if (g_capped || !same(one, want, what)) {
            if (g_capped) printf("FAIL %s: a loop ran past 4 N N passes\n", what);
            return 1;
          }
          snprintf(what, sizeof what, "%s N=%d conn=%d seed=%d threads", q.name.c_str(), N, conn, (int)seed);
          const Result many = run<std::atomic<uint32_t>>(q, N, conn, seed * 977 + (uint64_t)N, 8);
          if (g_capped || !same(many, want, what)) {
            if (g_capped) printf("FAIL %s: a loop ran past 4 N N passes\n", what);
            return 1;
          }
          cases += 2;
        }
      }
  }
  if (!seen[0] || !seen[1] || !seen[2] || !seen[3]) {
    printf("FAIL: the sequences never showed front %u, jump %u, secondary %u or a focus %u\n", seen[0], seen[1], seen[2],
           seen[3]);
    return 1;
  }
  printf("ok %d\n", cases);
  return 0;
}
