"""numpy replay of the arithmetic of ps_mcerr_* / predictive.MonteCarloError: add with its split at the batch
boundaries, close, finish and merge, one rounded operation per statement, so that the device's gmean and every
count can be compared bit for bit (gM2 and wM2 not: the device contracts the last product of its Welford step
into an fma, as sens_ref notes; nor a merge, whose products contract too); the derived maps and the split R-hat
formula; and the two-pass batch means they are checked against.  Shared by the CPU and GPU tests."""
import numpy as np


def new_state(shape, thresholds, b):
    k = len(thresholds)
    z = lambda: np.zeros(shape)
    return {'thr': [float(t) for t in thresholds], 'b': int(b), 'B': 0, 'open': 0, 'discarded': 0, 'members': 0,
            'bmean': z(), 'bM2': z(), 'gmean': z(), 'gM2': z(), 'wM2': z(),
            'bcnt': np.zeros((k,) + tuple(shape), dtype=np.uint64),
            's1': np.zeros((k,) + tuple(shape), dtype=np.uint64),
            's2': np.zeros((k,) + tuple(shape), dtype=np.uint64)}


def _step(mean, M2, W, v, w):
    """one weighted Welford step (the statements of sens_ref.add) -> (mean, M2)"""
    w = float(w)
    Wn = float(W + w)
    d = v - mean
    ch = d != 0.0
    t = d * w
    t = t / Wn
    mean1 = np.where(ch, mean + t, mean)
    wd = w * d
    r = v - mean1
    return mean1, np.where(ch, M2 + wd * r, M2)


def close(st):
    """the open batch becomes closed batch B + 1"""
    st['gmean'], st['gM2'] = _step(st['gmean'], st['gM2'], st['B'], st['bmean'], 1)
    st['wM2'] = st['wM2'] + st['bM2']
    st['s1'] += st['bcnt']
    st['s2'] += st['bcnt'] * st['bcnt']
    st['bmean'] = np.zeros_like(st['bmean'])
    st['bM2'] = np.zeros_like(st['bM2'])
    st['bcnt'][...] = 0
    st['B'] += 1
    st['open'] = 0


def add_piece(st, v, w):
    """a weight that fits the open batch"""
    assert 1 <= w <= st['b'] - st['open']
    st['bmean'], st['bM2'] = _step(st['bmean'], st['bM2'], st['open'], v, w)
    for k, t in enumerate(st['thr']):
        st['bcnt'][k] += np.uint64(w) * (v >= t).astype(np.uint64)
    st['open'] += w
    if st['open'] == st['b']:
        close(st)


def pieces(open_weight, b, w):
    """the library's split of a weight: fill the open batch, whole batches of b, the rest"""
    out = []
    while w > 0:
        p = min(w, b - open_weight)
        out.append(p)
        w -= p
        open_weight = (open_weight + p) % b
    return out


def add(st, v, w):
    """one member: field v with integer weight w >= 1"""
    v = np.asarray(v, dtype=np.float64)
    for p in pieces(st['open'], st['b'], int(w)):
        add_piece(st, v, p)
    st['members'] += 1
    return st


def finish(st):
    st['discarded'] += st['open']
    st['open'] = 0
    st['bmean'] = np.zeros_like(st['bmean'])
    st['bM2'] = np.zeros_like(st['bM2'])
    st['bcnt'][...] = 0
    return st


def merge(dst, src):
    """dst += src by Chan et al. with the batch counts (the expressions of ps_summary_merge, uncontracted)"""
    assert dst['open'] == 0 and src['open'] == 0 and dst['b'] == src['b']
    if src['B'] and not dst['B']:
        for key in ('gmean', 'gM2', 'wM2', 's1', 's2'):
            dst[key] = src[key].copy()
    elif src['B']:
        Ba, Bb = float(dst['B']), float(src['B'])
        B = Ba + Bb
        d = src['gmean'] - dst['gmean']
        t = d * (Bb / B)
        dst['gmean'] = dst['gmean'] + t
        q = dst['gM2'] + src['gM2']
        dd = d * d
        dst['gM2'] = q + dd * (Ba * Bb / B)
        dst['wM2'] = dst['wM2'] + src['wM2']
        dst['s1'] = dst['s1'] + src['s1']
        dst['s2'] = dst['s2'] + src['s2']
    dst['B'] += src['B']
    dst['discarded'] += src['discarded']
    dst['members'] += src['members']
    return dst


# ---- derived maps (B batches of weight b, n = b B)
def used(st):
    return st['b'] * st['B']


def mcse(st):
    B = float(st['B'])
    return np.sqrt(st['gM2'] / (B - 1.0) / B)


def variance(st):
    return (st['wM2'] + float(st['b']) * st['gM2']) / float(used(st))


def ess(st):
    B, b, n = float(st['B']), float(st['b']), float(used(st))
    out = np.zeros_like(st['gM2'])
    np.divide(n * variance(st), b * (st['gM2'] / (B - 1.0)), out=out, where=st['gM2'] != 0.0)
    return out


def count_variance_numerator(st, k):
    """B s2 - s1^2 as exact Python integers"""
    return st['B'] * st['s2'][k].astype(object) - st['s1'][k].astype(object) ** 2


def prob_mcse(st, k):
    B, b = float(st['B']), float(st['b'])
    return np.sqrt(count_variance_numerator(st, k).astype(np.float64) / (B * (B - 1.0)) / (b * b) / B)


def rhat(planes, b):
    """split R-hat from [(gmean, gM2, wM2, n)] per sequence, in that order"""
    nh = len(planes)
    s2 = [(w + float(b) * g) / (float(n) - 1.0) for _m, g, w, n in planes]
    W = sum(s2[1:], s2[0]) / float(nh)
    mbar = sum([p[0] for p in planes[1:]], planes[0][0]) / float(nh)
    Bv = sum([(p[0] - mbar) ** 2 for p in planes[1:]], (planes[0][0] - mbar) ** 2) / float(nh - 1)
    nbar = sum(float(p[3]) for p in planes) / float(nh)
    out = np.zeros_like(W)
    np.divide((nbar - 1.0) / nbar * W + Bv, W, out=out, where=W != 0.0)
    return np.sqrt(out)


def state_planes(st):
    return st['gmean'], st['gM2'], st['wM2'], used(st)


def two_pass(rows, b, thresholds=()):
    """closed-form batch means of the row series rows [n, ...] (one entry per row of weight), the remainder
    n % b dropped -> dict of mean, mcse, variance, ess, and per threshold (s1, s2, prob_mcse)"""
    rows = np.asarray(rows, dtype=np.float64)
    B = rows.shape[0] // b
    n = B * b
    x = rows[:n].reshape((B, b) + rows.shape[1:])
    bm = x.mean(1)
    mean = bm.mean(0)
    var_bm = ((bm - mean) ** 2).sum(0) / (B - 1.0)
    variance_ = ((rows[:n] - mean) ** 2).sum(0) / n
    ess_ = np.zeros_like(mean)
    np.divide(n * variance_, b * var_bm, out=ess_, where=var_bm != 0.0)
    out = {'B': B, 'n': n, 'mean': mean, 'mcse': np.sqrt(var_bm / B), 'variance': variance_, 'ess': ess_, 'thr': []}
    for t in thresholds:
        c = (x >= t).sum(1)
        p = c / float(b)
        var_p = ((p - p.mean(0)) ** 2).sum(0) / (B - 1.0)
        out['thr'].append((c.sum(0), (c.astype(np.int64) ** 2).sum(0), np.sqrt(var_p / B)))
    return out
