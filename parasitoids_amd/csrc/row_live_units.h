// Live units of a forward row pass whose source rows are confined to a range (a day kernel's blob
// inside its K x K box): which groups of `g` consecutive torus rows hold at least one row that the
// pass's row map sends into the inclusive source range [lo, hi].  The map (SrcMap of fft_kernels.h,
// here as plain integers so that host code without a device can call it) has two pieces,
//   r <  n1  -> r + off1          r >= lo2 -> r - lo2 + off2          everything else: zero,
// so the live torus rows are at most two intervals and the live groups at most two runs.  With
// map_wrap(M, P) these are [0, hi - M] and [P - M + lo, P - 1], clipped.
// The persistent row kernel (k_row_fwd_rsp) walks this list; its launcher sizes the grid with it.
#pragma once
#include "fft_core.h"

struct LiveRuns {   // groups [u0, u0 + c0) and [u1, u1 + c1), the second run above the first
  int u0, c0, u1, c1;
};

PS_HD LiveRuns live_runs(int n1, int off1, int lo2, int off2, int P, int lo, int hi, int g) {
  LiveRuns r{0, 0, 0, 0};
  if (lo > hi) return r;
  const int e1 = (n1 < P ? n1 : P) - 1;                  // last torus row of the first piece
  const int a = lo - off1 > 0 ? lo - off1 : 0, b = hi - off1 < e1 ? hi - off1 : e1;
  const int s2 = lo2 > n1 ? lo2 : n1;                    // the first piece wins where they overlap
  int c = lo - off2 + lo2, d = hi - off2 + lo2;
  c = c > s2 ? c : s2;
  c = c > 0 ? c : 0;
  d = d < P - 1 ? d : P - 1;
  if (a <= b) {
    r.u0 = a / g;
    r.c0 = b / g - r.u0 + 1;
  }
  if (c <= d) {
    int s = c / g;
    const int e = d / g;
    if (r.c0 && s < r.u0 + r.c0) s = r.u0 + r.c0;        // the runs touch: count the shared group once
    if (s <= e) {
      r.u1 = s;
      r.c1 = e - s + 1;
    }
  }
  return r;
}
PS_HD int live_count(const LiveRuns& r) { return r.c0 + r.c1; }
PS_HD int live_unit(const LiveRuns& r, int k) { return k < r.c0 ? r.u0 + k : r.u1 + (k - r.c0); }

// live groups of `count` batch entries, ranges = [count][2]
template <class RP>
PS_HD int live_total(int n1, int off1, int lo2, int off2, int P, RP ranges, int count, int g) {
  int t = 0;
  for (int d = 0; d < count; ++d) t += live_count(live_runs(n1, off1, lo2, off2, P, ranges[2 * d], ranges[2 * d + 1], g));
  return t;
}

// Position in the concatenated list -> (batch entry, group).  A cursor, because every caller walks the
// list upwards: advance() costs the entries it passes, once.
struct LiveCursor {
  int day, base;   // groups of the entries before `day`
  LiveRuns runs;   // of `day` (empty when day == count)
};
template <class RP>
PS_HD LiveCursor live_cursor(int n1, int off1, int lo2, int off2, int P, RP ranges, int count, int g) {
  LiveCursor c{0, 0, LiveRuns{0, 0, 0, 0}};
  if (count > 0) c.runs = live_runs(n1, off1, lo2, off2, P, ranges[0], ranges[1], g);
  return c;
}
// false: k is past the end of the list
template <class RP>
PS_HD bool live_advance(LiveCursor& c, int k, int n1, int off1, int lo2, int off2, int P, RP ranges, int count, int g) {
  while (c.day < count && k >= c.base + live_count(c.runs)) {
    c.base += live_count(c.runs);
    ++c.day;
    c.runs = c.day < count ? live_runs(n1, off1, lo2, off2, P, ranges[2 * c.day], ranges[2 * c.day + 1], g) : LiveRuns{0, 0, 0, 0};
  }
  return c.day < count;
}
