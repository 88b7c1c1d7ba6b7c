"""numpy reference of the reweighted excursion semantics of ps_wexcur_* / predictive.ReweightedExcursion for one plane
(one threshold, one slot), from the members' fields, their integer weights n, their log-weights and t.  The bits and
their packing are excur_ref's; everything after them is the statements of include/parasitoid_hip.h as plain loops
over the members in add order, one fp64 operation per statement and no multiply on the device's side: the device has
to reproduce every number bit for bit.  Shared by the CPU and GPU tests."""
import math

import numpy as np

import excur_ref as R


def member_weights(n, log_weights):
    """float64 [M]: w_m = n_m exp(l_m - max l), 0.0 at l_m = -inf (the definition of
    ReweightedArrival.member_weights, the reference the largest log-weight)"""
    lw = [float(v) for v in log_weights]
    ref = max(lw)
    assert ref > -math.inf and len(lw) == len(n)
    return np.array([0.0 if l == -math.inf else int(k) * math.exp(l - ref) for l, k in zip(lw, n)], dtype=np.float64)


def total(w):
    """W = w_0 + w_1 + ... in add order from 0.0"""
    W = 0.0
    for v in w:
        W = W + float(v)
    return W


def counts(B, w):
    """[ncell] float64: C = 0.0, then C += w_m where B_m, m in add order"""
    C = np.zeros(B.shape[1], dtype=np.float64)
    for m in range(B.shape[0]):
        C[B[m]] = C[B[m]] + w[m]
    return C


def bounds(B, C):
    """(hi [M], lo [M]) float64: hi_m = max{C(c) : B_m(c) = 0} (0.0 if none), lo_m = min{C(c) : B_m(c) = 1} (+inf)"""
    hi = np.zeros(len(B), dtype=np.float64)
    lo = np.full(len(B), np.inf, dtype=np.float64)
    for m, b in enumerate(B):
        if (~b).any():
            hi[m] = C[~b].max()
        if b.any():
            lo[m] = C[b].min()
    return hi, lo


def functions(C, hi, lo, w, W):
    """(F+, F-, Fc) float64 [ncell]: the sums over the members in add order from 0.0, then one division by W"""
    u = np.minimum(C, W - C)
    v = W - u
    Ap, Am, Ac = (np.zeros(C.shape, dtype=np.float64) for _ in range(3))
    for m in range(len(w)):
        sel = hi[m] < C
        Ap[sel] = Ap[sel] + w[m]
        sel = lo[m] > C
        Am[sel] = Am[sel] + w[m]
        sel = (hi[m] < v) & (lo[m] > u)
        Ac[sel] = Ac[sel] + w[m]
    Ap[C == 0.0] = 0.0
    Ac[u + u >= W] = 0.0
    return Ap / W, Am / W, Ac / W


def plane(fields, n, log_weights, t):
    """everything of one plane from the members' fields -> dict(B, w, W, C, hi, lo, above, below, contour, prob), the
    maps in the fields' own shape"""
    X = np.asarray(fields, dtype=np.float64)
    B = R.bits(X, t)
    w = member_weights(n, log_weights)
    W = total(w)
    C = counts(B, w)
    hi, lo = bounds(B, C)
    Fp, Fm, Fc = functions(C, hi, lo, w, W)
    shape = X.shape[1:]
    return {'B': B, 'w': w, 'W': W, 'C': C.reshape(shape), 'hi': hi, 'lo': lo, 'above': Fp.reshape(shape),
            'below': Fm.reshape(shape), 'contour': Fc.reshape(shape), 'prob': (C / W).reshape(shape)}
