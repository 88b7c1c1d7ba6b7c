// The per-thread logic of the patch maps (ps_patch.hip): which cells a cell is linked to, find, join and the key that
// picks the main patch.  Plain C++ that compiles for host and device: the kernels and the host emulation
// (tests/host/patch_emul.cpp) share it, and the atomic operations come in as the template parameter `At`:
//   uint32_t load(uint32_t i)                       parent[i], a read that sees other threads' joins
//   uint32_t cas(uint32_t i, uint32_t e, uint32_t d)   compare-and-swap on parent[i], returns the old value
//   bool     step()                                 called once per pass of every loop; false abandons the loop
//                                                   (the emulation's iteration cap; the device's returns true)
// The labelling is union-find on parent[c], one entry per cell of one plane: c for a cell of the set O when the link
// starts, PATCH_NONE outside O.  Invariant, throughout: parent[c] <= c for every c in O, and parent of a cell of O
// is a cell of O.  A join swaps a root only (compare-and-swap parent[a]: a -> b with b < a), so parent entries only
// ever fall, roots are never re-made, and the root of a finished patch is its smallest linear index -- the label.
// Every pass of every loop here either returns or strictly lowers an index; no thread waits for another's progress.
#pragma once
#include <stdint.h>

#ifndef PS_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PS_HD __host__ __device__ __forceinline__
#else
#define PS_HD inline
#endif
#endif

#define PATCH_NONE 0xffffffffu

// The neighbours of cell c = row * N + col that lie before it in linear order, under connectivity 4 (left, upper) or
// 8 (also upper-left and upper-right); each pair of adjacent cells is thus named once, by its later cell.  No wrap:
// column 0 has no left or upper-left neighbour (c - 1 is the previous row's last cell), column N - 1 no
// upper-right one, row 0 none above.  Returns how many of nb[0..3] are set.
PS_HD int patch_neighbours(uint32_t c, uint32_t N, int conn, uint32_t nb[4]) {
  const uint32_t row = c / N, col = c - row * N;
  int n = 0;
  if (col > 0) nb[n++] = c - 1;
  if (row > 0) {
    nb[n++] = c - N;
    if (conn == 8) {
      if (col > 0) nb[n++] = c - N - 1;
      if (col + 1 < N) nb[n++] = c - N + 1;
    }
  }
  return n;
}

// the root of c (a cell of O): walks parent until it stops falling.  p > c cannot happen under the invariant; it
// ends the walk too, so that no state of the array can keep a thread here.
template <class At>
PS_HD uint32_t patch_find(At& at, uint32_t c) {
  for (;;) {
    const uint32_t p = at.load(c);
    if (p >= c || !at.step()) return c;
    c = p;   // p < c
  }
}

// one patch out of those of a and b (cells of O).  Both roots are found, the larger, a, is swapped to point at the
// smaller if it still is a root; if it is not, the swap returned a parent below a and the pass starts again from
// there.  a + b falls strictly with every pass that does not return.
template <class At>
PS_HD void patch_join(At& at, uint32_t a, uint32_t b) {
  for (;;) {
    a = patch_find(at, a);
    b = patch_find(at, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    const uint32_t old = at.cas(a, a, b);
    if (old == a || old > a || !at.step()) return;   // old > a cannot happen (see patch_find)
    a = old;   // old < a
  }
}

// the link step of one cell of O: joined to each neighbour before it that lies in O
template <class At>
PS_HD void patch_link_cell(At& at, uint32_t c, uint32_t N, int conn) {
  uint32_t nb[4];
  const int n = patch_neighbours(c, N, conn, nb);
  for (int i = 0; i < n; ++i)
    if (at.load(nb[i]) != PATCH_NONE) patch_join(at, c, nb[i]);
}

// The main patch is the maximum of this key over the roots: the most cells, among equals the smallest label.
// A key of 0 (no root) unpacks to 0 cells and the label PATCH_NONE.
PS_HD uint64_t patch_key(uint32_t cells, uint32_t label) { return ((uint64_t)cells << 32) | (uint64_t)(0xffffffffu - label); }
PS_HD uint32_t patch_key_cells(uint64_t key) { return (uint32_t)(key >> 32); }
PS_HD uint32_t patch_key_label(uint64_t key) { return 0xffffffffu - (uint32_t)(key & 0xffffffffu); }
