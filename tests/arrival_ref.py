"""numpy reference of the arrival semantics of ps_arrival_* / predictive.ArrivalMaps: per member and cell the
first slot whose value reaches each threshold, the weighted counts of those slots, their running sums C,
arrival probabilities, arrival quantiles, the reached cells per member and slot, and weighted quantiles of
the reached area.  Shared by the CPU and GPU arrival tests."""
import numpy as np


def arrival_slots(fields, thresholds):
    """fields: [nslot, *shape] of one member -> [K, *shape] int64: a_k = min{s : v_s >= t_k}, nslot = never"""
    X = np.asarray(fields, dtype=np.float64)
    nslot = X.shape[0]
    out = []
    for t in thresholds:
        hit = X >= float(t)
        out.append(np.where(hit.any(0), np.argmax(hit, axis=0), nslot))
    return np.array(out, dtype=np.int64)


def weighted_counts(members, weights, thresholds):
    """members: [M][nslot, *shape] -> [K, nslot + 1, *shape] int64: the weight arriving at each slot, the last
    plane "never" """
    X0 = np.asarray(members[0])
    nslot, shape = X0.shape[0], X0.shape[1:]
    out = np.zeros((len(thresholds), nslot + 1) + shape, dtype=np.int64)
    for f, w in zip(members, weights):
        a = arrival_slots(f, thresholds)
        for k in range(len(thresholds)):
            for s in range(nslot + 1):
                out[k, s] += int(w) * (a[k] == s)
    return out


def cumulative(counts):
    """C_k[s] = the weight arrived by slot s (integers), [K, nslot, *shape]"""
    return np.cumsum(np.asarray(counts, dtype=np.int64)[:, :-1], axis=1)


def probability(counts):
    """P(arrived by slot s) = (double)C / (double)W"""
    counts = np.asarray(counts, dtype=np.int64)
    W = counts.sum(1)[:, None].astype(np.float64)
    return cumulative(counts).astype(np.float64) / W


def quantile_slots(counts, p):
    """[K, *shape]: the smallest s with (double)C_k[s] >= p * (double)W, -1 if even the last slot falls short"""
    counts = np.asarray(counts, dtype=np.int64)
    W = counts.sum(1).astype(np.float64)
    ok = cumulative(counts).astype(np.float64) >= p * W[:, None]
    return np.where(ok.any(1), np.argmax(ok, axis=1), -1)


def reached_rows(members, thresholds):
    """[M, K, nslot] int64: n_k(s) = #{c : a_k(c) <= s} per member"""
    rows = []
    for f in members:
        a = arrival_slots(f, thresholds).reshape(len(thresholds), -1)
        nslot = np.asarray(f).shape[0]
        rows.append([[int((a[k] <= s).sum()) for s in range(nslot)] for k in range(len(thresholds))])
    return np.array(rows, dtype=np.int64)


def area_quantile(values, weights, p):
    """min{a : sum of w_m over a_m <= a >= p W}, as (double)(integer weight) >= p * (double)W"""
    v = np.asarray(values)
    w = np.asarray(weights, dtype=np.int64)
    for a in np.unique(v):
        if float(w[v <= a].sum()) >= p * float(w.sum()):
            return a
    raise AssertionError('p > 1')
