// The per-thread logic of the proximity fields (ps_prox.hip): the distance along a row to the nearest bit of a
// set kept as 64-bit words, and the search down and up a column that turns those row distances into the exact
// squared Euclidean distance to the set.  Plain C++ that compiles for host and device: the kernels and the host
// emulation (tests/host/prox_emul.cpp) share it.  Integers throughout.
//   mask: bit c & 63 of word c >> 6 is cell c = y * N + x (the layout of ps_excur); a row's bits are lo .. hi
//   g(y, x): |x - x'| of the nearest set bit (y, x') of row y, PROX_NONE where the row holds none
//   d2(y, x) = min over y' of (y - y')^2 + g(y', x)^2, far2 where no row holds a bit
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

#define PROX_NONE 0xffffu        // a uint16 row distance no domain of N <= 32767 holds
#define PROX_MAX_N 32767         // 2 (N - 1)^2 + 1 fits 32 bits

// one more than any squared distance between two cells of the domain
PS_HD uint32_t prox_far2(int N) { return 2u * (uint32_t)(N - 1) * (uint32_t)(N - 1) + 1u; }

// the largest set bit b of the mask with lo <= b <= c, or -1: the own word below and at c first, then the words
// downwards to the one that holds lo
PS_HD int64_t prox_bit_at_or_below(const uint64_t* words, int64_t lo, int64_t c) {
  int64_t w = c >> 6;
  const int64_t wl = lo >> 6;
  uint64_t m = words[w] & (~0ull >> (63 - (int)(c & 63)));
  for (;;) {
    if (w == wl) m &= ~0ull << (int)(lo & 63);
    if (m) return (w << 6) + 63 - __builtin_clzll(m);
    if (w == wl) return -1;
    m = words[--w];
  }
}

// the smallest set bit b of the mask with c <= b <= hi, or -1
PS_HD int64_t prox_bit_at_or_above(const uint64_t* words, int64_t c, int64_t hi) {
  int64_t w = c >> 6;
  const int64_t wh = hi >> 6;
  uint64_t m = words[w] & (~0ull << (int)(c & 63));
  for (;;) {
    if (w == wh) m &= ~0ull >> (63 - (int)(hi & 63));
    if (m) return (w << 6) + __builtin_ctzll(m);
    if (w == wh) return -1;
    m = words[++w];
  }
}

// g of cell c of the row lo .. hi: the walk upwards goes no further than the bit found below
PS_HD uint32_t prox_row_dist(const uint64_t* words, int64_t lo, int64_t hi, int64_t c) {
  const int64_t below = prox_bit_at_or_below(words, lo, c);
  if (below == c) return 0u;
  int64_t top = hi;
  if (below >= 0 && c + (c - below) - 1 < top) top = c + (c - below) - 1;
  const int64_t above = prox_bit_at_or_above(words, c, top);
  if (above >= 0) return (uint32_t)(above - c);
  return below >= 0 ? (uint32_t)(c - below) : PROX_NONE;
}

// d2 of row y of one column: col[y' * stride] = g(y', x).  dy = 0, 1, 2, .. on both sides; it stops as soon as
// dy^2 >= the best so far (no further row can do better) or both sides have left the domain.
PS_HD uint32_t prox_col_search(const uint16_t* col, int64_t stride, int y, int N, uint32_t far2) {
  const uint32_t g0 = col[(int64_t)y * stride];
  uint32_t best = g0 == PROX_NONE ? far2 : g0 * g0;
  const int reach = y > N - 1 - y ? y : N - 1 - y;
  for (int dy = 1; dy <= reach; ++dy) {
    const uint32_t dd = (uint32_t)dy * (uint32_t)dy;
    if (dd >= best) break;
    if (y - dy >= 0) {
      const uint32_t g = col[(int64_t)(y - dy) * stride];
      if (g != PROX_NONE && dd + g * g < best) best = dd + g * g;
    }
    if (y + dy < N) {
      const uint32_t g = col[(int64_t)(y + dy) * stride];
      if (g != PROX_NONE && dd + g * g < best) best = dd + g * g;
    }
  }
  return best;
}

// the widest strip of columns, a power of two <= 64, whose g (N rows of uint16) fits `lds_bytes` of LDS
PS_HD int prox_strip_width(int N, int64_t lds_bytes) {
  int w = 64;
  while (w > 1 && (int64_t)w * N * 2 > lds_bytes) w >>= 1;
  return w;
}
