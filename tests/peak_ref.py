"""numpy reference of the peak semantics of ps_peak_* / predictive.PeakMaps, from [member][slot, *shape] fields:
per member and cell the peak value (np.maximum folded from a zero array in slot order), the first slot that
attains it ("none" where the peak is zero), the number of slots at or above each threshold, and over the members
the weighted counts, cumulative probabilities, the quantile rule and the mean duration.  Shared by the CPU and GPU
peak tests."""
import numpy as np


def peak_field(fields):
    """fields: [nslot, *shape] of one member -> [*shape]: m = max(+0.0, max_s v_s), folded in slot order"""
    X = np.asarray(fields, dtype=np.float64)
    m = np.zeros(X.shape[1:], dtype=np.float64)
    for s in range(X.shape[0]):
        m = np.maximum(m, X[s])
    return m


def peak_slot(fields):
    """[*shape] int64: the first slot that attains the peak (strict test v > m from m = +0.0), nslot = none"""
    X = np.asarray(fields, dtype=np.float64)
    nslot = X.shape[0]
    m = np.zeros(X.shape[1:], dtype=np.float64)
    p = np.full(X.shape[1:], nslot, dtype=np.int64)
    for s in range(nslot):
        up = X[s] > m
        m = np.where(up, X[s], m)
        p = np.where(up, s, p)
    return p


def durations(fields, thresholds):
    """[K, *shape] int64: dur_k = #{s : v_s >= t_k}"""
    X = np.asarray(fields, dtype=np.float64)
    out = np.zeros((len(thresholds),) + X.shape[1:], dtype=np.int64)
    for k, t in enumerate(thresholds):
        for s in range(X.shape[0]):
            out[k] += X[s] >= float(t)
    return out


def day_counts(members, weights):
    """[nslot + 1, *shape] int64: the weight peaking on each slot, the last plane "none" """
    nslot = np.asarray(members[0]).shape[0]
    out = np.zeros((nslot + 1,) + np.asarray(members[0]).shape[1:], dtype=np.int64)
    for f, w in zip(members, weights):
        p = peak_slot(f)
        for s in range(nslot + 1):
            out[s] += int(w) * (p == s)
    return out


def duration_counts(members, weights, thresholds):
    """[K, nslot + 1, *shape] int64: plane n the weight of the members with dur_k = n, n = 0 .. nslot"""
    nslot = np.asarray(members[0]).shape[0]
    out = np.zeros((len(thresholds), nslot + 1) + np.asarray(members[0]).shape[1:], dtype=np.int64)
    for f, w in zip(members, weights):
        d = durations(f, thresholds)
        for k in range(len(thresholds)):
            for n in range(nslot + 1):
                out[k, n] += int(w) * (d[k] == n)
    return out


def day_prob(dc):
    """[nslot, *shape]: P(peaked by slot s) = (double)(sum over s' <= s) / (double)W"""
    dc = np.asarray(dc, dtype=np.int64)
    W = float(dc.sum(0).flat[0])
    return np.cumsum(dc[:-1], axis=0).astype(np.float64) / W


def day_quantile(dc, p):
    """[*shape]: the smallest slot s with (double)C[s] >= p * (double)W, -1 if even the last slot falls short"""
    dc = np.asarray(dc, dtype=np.int64)
    W = float(dc.sum(0).flat[0])
    ok = np.cumsum(dc[:-1], axis=0).astype(np.float64) >= p * W
    return np.where(ok.any(0), np.argmax(ok, axis=0), -1)


def duration_prob(uc):
    """uc: [nslot + 1, *shape] of one threshold -> [nslot + 1, *shape]: plane n = P(dur >= n) (plane 0 is 1)"""
    uc = np.asarray(uc, dtype=np.int64)
    W = float(uc.sum(0).flat[0])
    return np.cumsum(uc[::-1], axis=0)[::-1].astype(np.float64) / W


def duration_quantile(uc, p):
    """[*shape]: the smallest n in 0..nslot whose cumulative count, n = 0 included, reaches p W"""
    uc = np.asarray(uc, dtype=np.int64)
    W = float(uc.sum(0).flat[0])
    ok = np.cumsum(uc, axis=0).astype(np.float64) >= p * W
    assert ok[-1].all()                    # C = W at n = nslot and p <= 1
    return np.argmax(ok, axis=0)


def duration_mean(uc):
    """[*shape]: (double)(sum over n of n * count_n) / (double)W, the sum in integers"""
    uc = np.asarray(uc, dtype=np.int64)
    W = float(uc.sum(0).flat[0])
    tot = np.zeros(uc.shape[1:], dtype=np.int64)
    for n in range(uc.shape[0]):
        tot += n * uc[n]
    return tot.astype(np.float64) / W
