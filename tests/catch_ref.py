"""numpy restatement of the catch-probability kernel (csrc/ps_catch.hip, catch_value), statement by statement
as include/parasitoid_hip.h fixes it: one IEEE double rounding per statement.  numpy never fuses, so each line
below is one of the header's statements; exp and expm1 are the host library's, which may differ from the
device's in the last bit."""
import numpy as np

TERMS = 56
SURE = 800.0


def catch_value(mu, n):
    '''P(Poisson(mu) >= n) for an array of mu and one whole n in 1..16'''
    n = int(n)
    if not 1 <= n <= 16:
        raise ValueError('count %r is not in 1..16' % (n,))
    mu = np.asarray(mu, dtype=np.float64)
    out = np.zeros(mu.shape, dtype=np.float64)
    out[mu >= SURE] = 1.0
    live = (mu > 0.0) & (mu < SURE)
    m = mu[live]
    if n == 1:
        x = np.expm1(-m)
        out[live] = -x
        return out
    e = np.exp(-m)
    y = np.empty_like(m)
    up = m < float(n)
    # the upper series: mu^n / n! as a running product, times 1 + sum_j prod mu / (n + j), times exp(-mu)
    a = m[up]
    t = np.ones_like(a)
    for i in range(1, n + 1):
        t = t * a
        t = t / float(i)
    s = np.ones_like(a)
    u = np.ones_like(a)
    for j in range(1, TERMS + 1):
        r = a / float(n + j)
        u = u * r
        s = s + u
    t = t * s
    ya = t * e[up]
    y[up] = np.where(ya > 1.0, 1.0, ya)
    # the lower sum: 1 - exp(-mu) sum_{i < n} mu^i / i!
    b = m[~up]
    u = np.ones_like(b)
    q = np.ones_like(b)
    for i in range(1, n):
        u = u * b
        u = u / float(i)
        q = q + u
    p = e[~up] * q
    yb = 1.0 - p
    y[~up] = np.where(yb < 0.0, 0.0, yb)
    out[live] = y
    return out


def catch_fields(v, rates, counts):
    '''[len(rates), ...]: the outputs of one apply over the value field v, mu = rate * v (one rounded product)'''
    v = np.asarray(v, dtype=np.float64)
    return np.stack([catch_value(np.float64(r) * v, n) for r, n in zip(rates, counts)])


def exact(mu, n, digits=60):
    '''mpmath at `digits` digits: P(Poisson(mu) >= n) = the regularised lower incomplete gamma P(n, mu), at the
    fp64 mu, as mpf'''
    import mpmath
    with mpmath.workdps(digits):
        return [mpmath.gammainc(n, 0, mpmath.mpf(float(x)), regularized=True) if x > 0 else mpmath.mpf(0)
                for x in np.asarray(mu, dtype=np.float64).ravel()]


def rel_errors(got, mu, n, floor=1e-290, digits=60):
    '''per entry |got - exact| / exact, and where exact < floor the absolute error instead'''
    import mpmath
    got = np.asarray(got, dtype=np.float64).ravel()
    ex = exact(mu, n, digits)
    err = np.empty(got.size)
    with mpmath.workdps(digits):
        for k, (g, x) in enumerate(zip(got, ex)):
            d = abs(mpmath.mpf(float(g)) - x)
            err[k] = float(d if x < floor else d / x)
    return err
