// P(Poisson(mu) >= n), the tail series of the catch-probability fields, shared by ps_catch.hip and ps_gain.hip so
// that both give the same bits for the same (mu, n).
#pragma once
#include <math.h>

#include <hip/hip_runtime.h>

#define PS_CATCH_MAX_COUNT 16
#define PS_CATCH_TERMS 56      // of the upper series: enough for count <= 16 at mu -> count
#define PS_CATCH_SURE 800.0    // exp(-mu) == 0 from 746 on: the value is 1.0 exactly

// P(Poisson(mu) >= n), n in 1..16; every step a statement of its own (one rounding each), as the header states
// them and tests/catch_ref.py repeats them.  The series stops where a term no longer changes the sum: every
// later term is smaller (mu < n), so the 56 terms of the restatement give the same bits.
__device__ inline double catch_value(double mu, int n) {
  if (!(mu > 0.0)) return 0.0;
  if (mu >= PS_CATCH_SURE) return 1.0;
  const double nm = -mu;
  if (n == 1) {
    const double x = expm1(nm);
    return -x;
  }
  const double e = exp(nm);
  if (mu < (double)n) {
    double t = 1.0;
    for (int i = 1; i <= n; ++i) {
      t = t * mu;
      t = t / (double)i;
    }
    double s = 1.0, u = 1.0;
    for (int j = 1; j <= PS_CATCH_TERMS; ++j) {
      const double r = mu / (double)(n + j);
      u = u * r;
      const double s1 = s + u;
      if (s1 == s) break;
      s = s1;
    }
    t = t * s;
    const double y = t * e;
    return y > 1.0 ? 1.0 : y;
  }
  double u = 1.0, q = 1.0;
  for (int i = 1; i < n; ++i) {
    u = u * mu;
    u = u / (double)i;
    q = q + u;
  }
  const double p = e * q;
  const double y = 1.0 - p;
  return y < 0.0 ? 0.0 : y;
}
