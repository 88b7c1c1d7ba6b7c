"""numpy reference of the histogram semantics of ps_hist_* / predictive.SpreadHistogram: bins, weighted
counts, quantile index, point value, bracket and exceedance, and the exact weighted lower quantile of the
values themselves.  Shared by the CPU and GPU histogram tests."""
import numpy as np


def weighted_counts(fields, weights, edges):
    """[B + 2, *shape] int64: per cell the weight of every bin b = searchsorted(edges, v, side='right')"""
    edges = np.asarray(edges, dtype=np.float64)
    shape = np.shape(fields[0])
    out = np.zeros((edges.size + 1, int(np.prod(shape))), dtype=np.int64)
    cells = np.arange(out.shape[1])
    for f, w in zip(fields, weights):
        b = np.searchsorted(edges, np.asarray(f, dtype=np.float64).ravel(), side='right')
        out[b, cells] += int(w)
    return out.reshape((edges.size + 1,) + shape)


def quantile_from_counts(counts, edges, p):
    """-> (b*, value, lower, upper) per cell: b* = the smallest b with (double)C_b >= p * (double)W"""
    edges = np.asarray(edges, dtype=np.float64)
    B1 = edges.size                                      # B + 1
    counts = np.asarray(counts, dtype=np.int64)
    C = np.cumsum(counts, axis=0)
    W = C[-1]
    pW = p * W.astype(np.float64)
    bstar = np.argmax(C.astype(np.float64) >= pW, axis=0)
    lower = np.concatenate([[0.0], edges])[bstar]
    upper = np.concatenate([edges, [np.inf]])[bstar]
    value = np.zeros(bstar.shape)
    value[bstar == B1] = edges[-1]
    mid = (bstar >= 1) & (bstar <= B1 - 1)
    b = bstar[mid]
    Cm = np.take_along_axis(C, (bstar - 1).clip(0)[None], 0)[0][mid].astype(np.float64)
    cnt = np.take_along_axis(counts, bstar[None], 0)[0][mid].astype(np.float64)
    f = (pW[mid] - Cm) / cnt
    el, eh = edges[b - 1], edges[b]
    value[mid] = el * (eh / el) ** f
    return bstar, value, lower, upper


def exceedance_from_counts(counts, k):
    """P(v >= e_k) = (W - C_k) / W per cell"""
    counts = np.asarray(counts, dtype=np.int64)
    W = counts.sum(0).astype(np.float64)
    return counts[k + 1:].sum(0).astype(np.float64) / W


def exact_quantile(fields, weights, p):
    """min{v : F(v) >= p} per cell over the members' values, F the weighted distribution function,
    compared as (double)(integer weight <= v) >= p * (double)W"""
    X = np.asarray(fields, dtype=np.float64).reshape(len(fields), -1)
    w = np.asarray(weights, dtype=np.int64)
    order = np.argsort(X, axis=0, kind='stable')
    Xs = np.take_along_axis(X, order, 0)
    Cw = np.cumsum(w[order], axis=0)
    # the first sorted position whose running weight reaches p W holds the quantile (a tie before it
    # has the same value)
    j = np.argmax(Cw.astype(np.float64) >= p * float(w.sum()), axis=0)
    return Xs[j, np.arange(X.shape[1])].reshape(np.shape(fields[0]))
