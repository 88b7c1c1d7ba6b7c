"""Numpy reference of the reweighted summaries (ps_wsum_*, predictive.ReweightedSummary): the log-scale
bookkeeping with math.exp, the per-cell loop with one rounded operation per statement -- so that mean and every
exceedance sum come out with the device's bits; M2 ends in a product-and-add the device contracts, and is compared
with a tolerance --, the merge, the probe log-likelihoods, the run formula and the weight diagnostics.  It shares
no code with the package."""
import math

import numpy as np


def new_state(shape, thresholds, nscen):
    """shape: [nslot, N, N] of one member's fields"""
    return [{'W': 0.0, 'ref': -math.inf, 'members': 0, 'skipped': 0, 'thr': [float(t) for t in thresholds],
             'mean': np.zeros(shape), 'q': np.zeros(shape), 'S': [np.zeros(shape) for _ in thresholds]}
            for _ in range(nscen)]


def scale(ref, lam, weight):
    """(r, omega, new ref) of one scenario for a member with log-weight lam"""
    w = float(weight)
    if lam == -math.inf:
        return 1.0, 0.0, ref
    if ref == -math.inf:
        return 1.0, w, lam
    if lam > ref:
        return math.exp(ref - lam), w, lam
    return 1.0, w * math.exp(lam - ref), ref


def add(state, fields, lams, weight=1):
    v = np.asarray(fields, dtype=np.float64)
    for sc, lam in zip(state, lams):
        r, om, ref = scale(sc['ref'], float(lam), weight)
        if om == 0.0:
            sc['skipped'] += 1
            continue
        sc['ref'] = ref
        W = sc['W']
        W = W * r
        W = W + om
        m = sc['mean']
        q = sc['q'] * r
        S = [s * r for s in sc['S']]
        d = v - m
        t = d * om
        t = t / W
        m_new = m + t
        u = om * d
        z = v - m_new
        p = u * z                      # the device contracts this product into the sum: M2 is within an ulp or so
        q_new = q + p
        nz = d != 0.0
        sc['mean'] = np.where(nz, m_new, m)
        sc['q'] = np.where(nz, q_new, q)
        sc['S'] = [np.where(v >= tk, s + om, s) for tk, s in zip(sc['thr'], S)]
        sc['W'] = W
        sc['members'] += 1


def merge(dst, src):
    """dst += src per scenario, both brought to the larger reference; src unchanged"""
    for a, b in zip(dst, src):
        if b['W'] == 0.0:
            a['skipped'] += b['skipped']
            continue
        if a['W'] == 0.0:
            a['W'], a['ref'] = b['W'], b['ref']
            a['mean'], a['q'], a['S'] = b['mean'].copy(), b['q'].copy(), [s.copy() for s in b['S']]
        else:
            top = max(a['ref'], b['ref'])
            ra, rb = math.exp(a['ref'] - top), math.exp(b['ref'] - top)
            Wa = a['W'] * ra
            Wb = b['W'] * rb
            W = Wa + Wb
            d = b['mean'] - a['mean']
            a['mean'] = a['mean'] + d * (Wb / W)
            a['q'] = a['q'] * ra + b['q'] * rb + d * d * (Wa * Wb / W)
            a['S'] = [sa * ra + sb * rb for sa, sb in zip(a['S'], b['S'])]
            a['W'], a['ref'] = W, top
        a['members'] += b['members']
        a['skipped'] += b['skipped']


def mean(sc):
    return sc['mean']


def variance(sc):
    return sc['q'] / sc['W']


def exceedance(sc, k):
    return np.minimum(sc['S'][k] / sc['W'], 1.0)


def log_total_weight(sc):
    return -math.inf if sc['W'] == 0.0 else sc['ref'] + math.log(sc['W'])


def two_pass(fields, weights, lams, thresholds):
    """the plain definitions with normalised weights: fields [member, nslot, N, N] -> mean, variance,
    [exceedance per threshold]"""
    X = np.asarray(fields, dtype=np.float64)
    lam = np.asarray(lams, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64) * np.exp(lam - lam.max())
    w = w / w.sum()
    mu = np.tensordot(w, X, axes=1)
    var = np.tensordot(w, (X - mu[None]) ** 2, axes=1)
    exc = [np.tensordot(w, (X >= t).astype(np.float64), axes=1) for t in thresholds]
    return mu, var, exc


def probe_loglik(kind, rate, v, n=None):
    mu = rate * v
    if kind == 'none':
        return -mu
    if kind == 'found':
        if mu == 0.0:
            return -math.inf
        return math.log(-math.expm1(-mu)) if mu <= math.log(2.0) else math.log1p(-math.exp(-mu))
    assert kind == 'count'
    if mu == 0.0:
        return 0.0 if n == 0 else -math.inf
    return n * math.log(mu) - mu - math.lgamma(n + 1)


def probes_loglik(probes, values):
    """probes: (east, north, day, kind, rate[, n]) tuples; the sum in list order from 0.0"""
    lam = 0.0
    for p, v in zip(probes, values):
        lam = lam + probe_loglik(p[3], float(p[4]), float(v), p[5] if len(p) > 5 else None)
    return lam


def run_log_weight(ls):
    ls = [float(v) for v in ls]
    mx = max(ls)
    if mx == -math.inf:
        return -math.inf
    s = 0.0
    for v in ls:
        s = s + math.exp(v - mx)
    return mx + math.log(s / len(ls))


def diagnostics(row_logw):
    l = np.asarray(row_logw, dtype=np.float64)
    mx = l.max()
    e = np.exp(l - mx)
    s1, s2 = float(e.sum()), float((e * e).sum())
    return {'rows': int(l.size), 'skipped_rows': int((e == 0.0).sum()), 'ess': s1 * s1 / s2,
            'max_share': float(e.max()) / s1, 'log_mean_weight': float(mx + np.log(s1) - np.log(l.size))}
