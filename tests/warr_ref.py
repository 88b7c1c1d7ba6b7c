"""Numpy reference of the reweighted arrival maps (ps_warr_*, predictive.ReweightedArrival): the planes of real
weights per threshold and arrival slot with one rounded operation per statement, so that every plane comes out with
the device's bits; the running sums, arrival probabilities and quantile slots from the planes by the device's own
recurrence (C_s = C_{s-1} + A_s ascending); and the merge.  The (r, omega, ref) rule is reweight_ref's, the arrival
slot arrival_ref's.  It shares no code with the package."""
import math

import numpy as np

import reweight_ref as RR
from arrival_ref import arrival_slots


def new_state(shape, thresholds, nscen):
    """shape: [nslot, N, N] of one member's fields; A[k][s] the plane of threshold k and arrival slot s"""
    thr = [float(t) for t in thresholds]
    return [{'W': 0.0, 'ref': -math.inf, 'members': 0, 'skipped': 0, 'thr': thr,
             'A': np.zeros((len(thr),) + tuple(shape))} for _ in range(nscen)]


def add(state, fields, lams, weight=1):
    a = arrival_slots(fields, state[0]['thr'])           # [K, N, N], nslot = never
    for sc, lam in zip(state, lams):
        r, om, ref = RR.scale(sc['ref'], float(lam), weight)
        if om == 0.0:
            sc['skipped'] += 1
            continue
        sc['ref'] = ref
        W = sc['W']
        W = W * r
        W = W + om
        A = sc['A']
        if r != 1.0:
            A = A * r
        for k in range(A.shape[0]):
            for s in range(A.shape[1]):
                A[k, s] = np.where(a[k] == s, A[k, s] + om, A[k, s])
        sc['A'] = A
        sc['W'] = W
        sc['members'] += 1


def merge(dst, src):
    """dst += src per scenario, both brought to the larger reference; src unchanged"""
    for a, b in zip(dst, src):
        if b['W'] == 0.0:
            a['skipped'] += b['skipped']
            continue
        if a['W'] == 0.0:
            a['W'], a['ref'], a['A'] = b['W'], b['ref'], b['A'].copy()
        else:
            top = max(a['ref'], b['ref'])
            ra, rb = math.exp(a['ref'] - top), math.exp(b['ref'] - top)
            Wa = a['W'] * ra
            Wb = b['W'] * rb
            x = a['A'] * ra
            y = b['A'] * rb
            a['A'] = x + y
            a['W'], a['ref'] = Wa + Wb, top
        a['members'] += b['members']
        a['skipped'] += b['skipped']


def cumulative(A):
    """A: [nslot, ...] the planes of one scenario and threshold -> C[s] = C[s - 1] + A[s], one rounded add each"""
    A = np.asarray(A, dtype=np.float64)
    C = np.zeros_like(A)
    run = np.zeros(A.shape[1:])
    for s in range(A.shape[0]):
        run = run + A[s]
        C[s] = run
    return C


def probability(A, W):
    """min(C_s / W, 1.0) per slot"""
    return np.minimum(cumulative(A) / W, 1.0)


def quantile_slots(A, W, p):
    """the smallest s with C_s >= p W, -1 if even the last slot falls short"""
    ok = cumulative(A) >= p * W
    return np.where(ok.any(0), np.argmax(ok, axis=0), -1)
