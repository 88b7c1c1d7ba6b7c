"""numpy restatement of the trap information kernels (csrc/ps_gain.hip: k_gain_apply, k_gain_finish), statement by
statement as include/parasitoid_hip.h fixes them: one IEEE double rounding per statement, on top of
catch_ref.catch_value.  numpy never fuses, so each line below is one of the header's statements; exp, expm1 and log
are the host library's, which may differ from the device's in the last bit."""
import numpy as np

import catch_ref

SURE = catch_ref.SURE
MAX_YMAX = 15


def _minus_xlogx(h, p):
    '''h = h - x with l = log(p), x = p * l, where p > 0; h as it is elsewhere'''
    pos = p > 0.0
    l = np.log(p[pos])
    x = p[pos] * l
    h = h.copy()
    h[pos] = h[pos] - x
    return h


def apply(mu, ymax):
    '''[ymax + 3, ...]: the planes d0, p_1 .. p_ymax, tail, h of one trap for an array of mu'''
    ymax = int(ymax)
    if not 0 <= ymax <= MAX_YMAX:
        raise ValueError('ymax %r is not in 0..%d' % (ymax, MAX_YMAX))
    mu = np.asarray(mu, dtype=np.float64)
    out = np.zeros((ymax + 3,) + mu.shape, dtype=np.float64)
    sure = mu >= SURE
    out[0][sure] = 1.0
    out[ymax + 1][sure] = 1.0
    live = (mu > 0.0) & (mu < SURE)
    m = mu[live]
    nm = -m
    x = np.expm1(nm)
    out[0][live] = -x
    e = np.exp(nm)
    h = e * m
    t = e
    for y in range(1, ymax + 1):
        t = t * m
        t = t / float(y)
        out[y][live] = t
        h = _minus_xlogx(h, t)
    q = catch_ref.catch_value(m, ymax + 1)
    out[ymax + 1][live] = q
    h = _minus_xlogx(h, q)
    out[ymax + 2][live] = h
    return out


def fields(v, rate, ymax):
    '''the planes of one trap over the value field v, mu = rate * v (one rounded product)'''
    return apply(np.float64(rate) * np.asarray(v, dtype=np.float64), ymax)


def finish(m):
    '''(gain, entropy, conditional) from the mean planes m [ymax + 3, ...] of one trap'''
    m = np.asarray(m, dtype=np.float64)
    ymax = m.shape[0] - 3
    P0 = 1.0 - m[0]
    HY = np.zeros(m.shape[1:], dtype=np.float64)
    for P in [P0] + [m[k] for k in range(1, ymax + 2)]:
        HY = _minus_xlogx(HY, P)
    HYM = m[ymax + 2]
    G = HY - HYM
    G = np.where(G > 0.0, G, 0.0)
    return G, HY, HYM.copy()


def weighted_mean(planes, weights):
    '''the weighted mean over axis 0 of planes [members, ...], by the Welford statements of the accumulators
    (sum_update): d = v - m; m += d * w / W'''
    planes = np.asarray(planes, dtype=np.float64)
    m = np.zeros(planes.shape[1:], dtype=np.float64)
    W = 0.0
    for v, w in zip(planes, weights):
        W = W + float(w)
        d = v - m
        m = m + d * float(w) / W
    return m


def cap(weights):
    '''the entropy in nats of the normalised member weights: no finite ensemble can show a larger gain'''
    w = np.asarray(weights, dtype=np.float64)
    w = w[w > 0.0]
    p = w / w.sum()
    return float(-(p * np.log(p)).sum())


def exact(mu, ymax, digits=60):
    '''mpmath at `digits` digits, at the fp64 mu: per entry the list [d0, p_1 .. p_ymax, tail, h] as mpf'''
    import mpmath
    out = []
    with mpmath.workdps(digits):
        for x in np.asarray(mu, dtype=np.float64).ravel():
            if not x > 0:
                out.append([mpmath.mpf(0)] * (ymax + 3))
                continue
            m = mpmath.mpf(float(x))
            e = mpmath.exp(-m)
            p = [e * m ** y / mpmath.factorial(y) for y in range(ymax + 1)]
            tail = mpmath.gammainc(ymax + 1, 0, m, regularized=True)
            h = -sum(c * mpmath.log(c) for c in p + [tail] if c > 0)
            out.append([-mpmath.expm1(-m)] + p[1:] + [tail, h])
    return out


def errors(got, mu, ymax, floor=1e-290, digits=60, ex=None):
    '''(rel [ymax + 2, n], abs_h [n]): per class plane |got - exact| / exact (the absolute error where exact <
    floor), and the absolute error of h; ex: the result of exact(mu, ymax), to share it between two calls'''
    import mpmath
    got = np.asarray(got, dtype=np.float64).reshape(ymax + 3, -1)
    if ex is None:
        ex = exact(mu, ymax, digits)
    rel = np.empty((ymax + 2, got.shape[1]))
    ah = np.empty(got.shape[1])
    with mpmath.workdps(digits):
        for k, row in enumerate(ex):
            for p in range(ymax + 2):
                d = abs(mpmath.mpf(float(got[p, k])) - row[p])
                rel[p, k] = float(d if row[p] < floor else d / row[p])
            ah[k] = float(abs(mpmath.mpf(float(got[ymax + 2, k])) - row[ymax + 2]))
    return rel, ah
