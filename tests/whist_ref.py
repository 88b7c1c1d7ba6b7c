"""Numpy reference of the reweighted histograms (ps_whist_*, predictive.ReweightedHistogram): the planes of real
weights on fixed edges with one rounded operation per statement, so that every plane comes out with the device's
bits; the quantile bin, bracket, point value and exceedance from the planes by the device's own recurrences
(T_b = T_{b+1} + H_b from the top, C_b = W - T_{b+1}); and the merge.  The (r, omega, ref) rule is reweight_ref's.
It shares no code with the package."""
import math

import numpy as np

import reweight_ref as RR


def new_state(shape, edges, nscen):
    """shape: [nslot, N, N] of one member's fields; H[b] is the plane of bin b = 0 .. B + 1, H[0] never written"""
    e = np.asarray(edges, dtype=np.float64)
    return [{'W': 0.0, 'ref': -math.inf, 'members': 0, 'skipped': 0, 'edges': e,
             'H': np.zeros((e.size + 1,) + tuple(shape))} for _ in range(nscen)]


def bins(fields, edges):
    return np.searchsorted(np.asarray(edges, dtype=np.float64), np.asarray(fields, dtype=np.float64), side='right')


def add(state, fields, lams, weight=1):
    v = np.asarray(fields, dtype=np.float64)
    for sc, lam in zip(state, lams):
        r, om, ref = RR.scale(sc['ref'], float(lam), weight)
        if om == 0.0:
            sc['skipped'] += 1
            continue
        sc['ref'] = ref
        W = sc['W']
        W = W * r
        W = W + om
        H = sc['H']
        if r != 1.0:
            H = H * r
        b = bins(v, sc['edges'])
        for k in range(1, H.shape[0]):
            H[k] = np.where(b == k, H[k] + om, H[k])
        sc['H'] = H
        sc['W'] = W
        sc['members'] += 1


def merge(dst, src):
    """dst += src per scenario, both brought to the larger reference; src unchanged"""
    for a, b in zip(dst, src):
        if b['W'] == 0.0:
            a['skipped'] += b['skipped']
            continue
        if a['W'] == 0.0:
            a['W'], a['ref'], a['H'] = b['W'], b['ref'], b['H'].copy()
        else:
            top = max(a['ref'], b['ref'])
            ra, rb = math.exp(a['ref'] - top), math.exp(b['ref'] - top)
            Wa = a['W'] * ra
            Wb = b['W'] * rb
            x = a['H'] * ra
            y = b['H'] * rb
            a['H'] = x + y
            a['W'], a['ref'] = Wa + Wb, top
        a['members'] += b['members']
        a['skipped'] += b['skipped']


def tails(H):
    """T[b] = T[b + 1] + H[b] for b = B + 1 .. 1, T[B + 2] = 0, T[0] = T[1] (bin 0 is not stored): [B + 3, ...]"""
    H = np.asarray(H, dtype=np.float64)
    T = np.zeros((H.shape[0] + 1,) + H.shape[1:])
    for b in range(H.shape[0] - 1, 0, -1):
        T[b] = T[b + 1] + H[b]
    T[0] = T[1]
    return T


def quantile_from_planes(H, W, edges, p):
    """H: [B + 2, ...] the planes of one scenario and slot (H[0] ignored) -> (b*, value, lower, upper, near):
    b* the smallest b with C_b >= p W, C_b = W - T_{b+1}; near: min over b of |C_b - p W| / W, how close the cell
    is to a tie"""
    edges = np.asarray(edges, dtype=np.float64)
    B1 = edges.size
    H = np.asarray(H, dtype=np.float64)
    T = tails(H)
    C = W - T[1:]                                        # C[b], b = 0 .. B + 1
    pW = p * W
    bstar = np.argmax(C >= pW, axis=0)
    lower = np.concatenate([[0.0], edges])[bstar]
    upper = np.concatenate([edges, [np.inf]])[bstar]
    value = np.zeros(bstar.shape)
    value[bstar == B1] = edges[-1]
    mid = (bstar >= 1) & (bstar <= B1 - 1)
    b = bstar[mid]
    Cm = np.take_along_axis(C, (bstar - 1).clip(0)[None], 0)[0][mid]
    c = np.take_along_axis(H, bstar[None], 0)[0][mid]
    f = (pW - Cm) / c
    f = np.where(f < 0.0, 0.0, f)
    f = np.where(f > 1.0, 1.0, f)
    el, eh = edges[b - 1], edges[b]
    value[mid] = el * (eh / el) ** f
    near = np.abs(C - pW).min(0) / W
    return bstar, value, lower, upper, near


def exceedance_from_planes(H, W, k):
    """min(T_{k+1} / W, 1.0): P(v >= e_k)"""
    return np.minimum(tails(H)[k + 1] / W, 1.0)


def exact_quantile(fields, weights, p):
    """min{v : F(v) >= p} per cell over the members' values under real weights, F the weighted distribution
    function: the running weight in the order of the sorted values against p times its last entry -> (quantile,
    near: the smallest |running weight - p W| / W of the cell)"""
    X = np.asarray(fields, dtype=np.float64).reshape(len(fields), -1)
    w = np.asarray(weights, dtype=np.float64)
    order = np.argsort(X, axis=0, kind='stable')
    Xs = np.take_along_axis(X, order, 0)
    Cw = np.cumsum(w[order], axis=0)
    W = Cw[-1]
    j = np.argmax(Cw >= p * W, axis=0)
    near = np.abs(Cw - p * W).min(0) / W
    shape = np.shape(fields[0])
    return Xs[j, np.arange(X.shape[1])].reshape(shape), near.reshape(shape)
