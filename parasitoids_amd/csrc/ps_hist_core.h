// The bin search and the range word of the per-cell histograms, shared by ps_hist.hip (integer counts) and
// ps_whist.hip (real weights) so that both put a value into the same bin and encode a cell's touched bins alike.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// searchsorted(e, v, side='right') over e[0..n): the number of edges <= v.  Comparisons only, no log.
__device__ inline int hist_bin(const double* e, int n, double v) {
  int lo = 0;
  while (n > 0) {
    const int half = n >> 1;
    if (e[lo + half] <= v) {
      lo += half + 1;
      n -= half + 1;
    } else {
      n = half;
    }
  }
  return lo;
}

// the range word (hi << 16) | (0xffff - lo) of a cell after bin b was touched; 0 = no bin yet
__device__ inline uint32_t hist_range_add(uint32_t r, int b) {
  const uint32_t hi = max(r >> 16, (uint32_t)b);
  const uint32_t lo = max(r & 0xffffu, 0xffffu - (uint32_t)b);
  return (hi << 16) | lo;
}
