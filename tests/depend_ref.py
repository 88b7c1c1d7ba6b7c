"""numpy replay of the arithmetic of ps_depend_* / predictive.DependenceMaps: add, merge and finalize with one
rounded operation per statement, so that the device's mean, bin sums, correlation ratios and dominant index can be
compared bit for bit; and the weighted two-pass correlation ratio straight from its definition, which the
tolerances are checked against.  Shared by the CPU and GPU dependence tests."""
import numpy as np


class Planes():
    """S[param][bin] planes that exist once they are written: 15 parameters x 16 bins of day fields are few planes
    that hold anything and gigabytes of zeros.  S[p, b] and S[p][b] read (zeros where nothing was written),
    S[p, b] = plane writes."""

    def __init__(self, nparam, nbin, shape):
        self.nparam, self.nbin, self.shape = nparam, nbin, tuple(shape)
        self.planes = {}
        self.zero = np.zeros(self.shape)
        self.zero.setflags(write=False)

    def __getitem__(self, key):
        if isinstance(key, tuple):
            p, b = int(key[0]), int(key[1])
            if not (0 <= p < self.nparam and 0 <= b < self.nbin):
                raise IndexError(key)
            return self.planes.get((p, b), self.zero)
        return [self[key, b] for b in range(self.nbin)]

    def __setitem__(self, key, plane):
        self[key]                                        # the index check
        self.planes[(int(key[0]), int(key[1]))] = np.asarray(plane, dtype=np.float64)

    def __add__(self, other):
        out = Planes(self.nparam, self.nbin, self.shape)
        for key in set(self.planes) | set(other.planes):
            out[key] = self[key] + other[key]
        return out

    def copy(self):
        out = Planes(self.nparam, self.nbin, self.shape)
        out.planes = {k: v.copy() for k, v in self.planes.items()}
        return out


def new_state(shape, nparam, nbin, dense=True):
    """dense=False: the planes of S as a Planes object instead of one array"""
    S = np.zeros((nparam, nbin) + tuple(shape)) if dense else Planes(nparam, nbin, shape)
    return {'W': 0, 'mean': np.zeros(shape), 'M2': np.zeros(shape), 'S': S,
            'Wb': np.zeros((nparam, nbin), dtype=np.int64), 'members': 0}


def add(state, v, bins, w):
    """one member: field v, bins[nparam] the bin of each of its scalars, integer weight w.  mean and every S plane
    follow the device bit for bit; M2 does not (the device contracts its last product into an fma, as ps_summary
    does).  The mean / M2 statements are those of sens_ref.add."""
    v = np.asarray(v, dtype=np.float64)
    wi = int(w)
    w = float(wi)
    Wn = float(state['W'] + wi)
    mean = state['mean']
    d = v - mean
    ch = d != 0.0
    t = d * w
    t = t / Wn
    mean1 = np.where(ch, mean + t, mean)
    wd = w * d
    r = v - mean1
    state['M2'] = np.where(ch, state['M2'] + wd * r, state['M2'])
    wv = w * v
    for p, b in enumerate(bins):
        state['S'][p, b] = state['S'][p, b] + wv
        state['Wb'][p, b] += wi
    state['mean'] = mean1
    state['W'] += wi
    state['members'] += 1
    return state


def merge(a, b):
    """a += b, the statements of ps_depend_merge in their order; into an empty a a copy"""
    if b['W'] == 0:
        return a
    if a['W'] == 0:
        for k in ('mean', 'M2', 'S', 'Wb'):
            a[k] = b[k].copy()
        a['W'], a['members'] = b['W'], b['members']
        return a
    Wa, Wb = float(a['W']), float(b['W'])
    W = Wa + Wb
    fb = Wb / W
    fab = Wa * Wb
    fab = fab / W
    d = b['mean'] - a['mean']
    t = d * fb
    a['mean'] = a['mean'] + t
    q = a['M2'] + b['M2']
    dd = d * d
    dd = dd * fab
    a['M2'] = q + dd
    a['S'] = a['S'] + b['S']
    a['Wb'] = a['Wb'] + b['Wb']
    a['W'] += b['W']
    a['members'] += b['members']
    return a


def finalize(mean, var, S, Wb):
    """(eta[nparam], dom) from the fetched maps mean, var = M2 / W, the planes S[nparam][nbin] and the integer bin
    weights Wb[nparam][nbin], every row of which sums to W: per parameter over the bins with Wb > 0 in ascending
    order s += Wb (S / Wb - mean)^2, eta = min((s / W) / var, 1), 0 where var == 0 or fewer than two bins hold a
    member; dom = the lowest p that
    maximises eta_p by a strict >, -1 where every eta_p is 0"""
    mean = np.asarray(mean, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    Wb = np.asarray(Wb)
    nparam, nbin = Wb.shape
    W = float(int(Wb[0].sum()))
    live = var != 0.0
    eta = np.zeros((nparam,) + var.shape)
    best = np.zeros(var.shape)
    dom = np.full(var.shape, -1, dtype=np.int8)
    for p in range(nparam):
        s = np.zeros(var.shape)
        for b in range(nbin):
            wb = float(int(Wb[p, b]))
            if wb > 0.0:
                mb = S[p][b] / wb
                d = mb - mean
                q = d * d
                q = wb * q
                s = s + q
        s = s / W
        e = np.zeros(var.shape)
        np.divide(s, var, out=e, where=live & (np.count_nonzero(Wb[p]) >= 2))
        e = np.minimum(e, 1.0)
        eta[p] = e
        up = e > best
        dom[up] = p
        best = np.where(up, e, best)
    return eta, dom


def ratio(fields, bins, weights):
    """the weighted correlation ratio straight from the definition, two passes: fields [member, *shape], bins
    [member] the bin of every member, weights [member] -> (eta2 [*shape], mean, variance); eta2 is 0 where the
    variance is 0"""
    X = np.asarray(fields, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    bins = np.asarray(bins)
    W = w.sum()
    mean = np.tensordot(w, X, axes=1) / W
    var = np.tensordot(w, (X - mean[None]) ** 2, axes=1) / W
    between = np.zeros(mean.shape)
    for b in np.unique(bins):
        sel = bins == b
        wb = w[sel].sum()
        mb = np.tensordot(w[sel], X[sel], axes=1) / wb
        between += wb * (mb - mean) ** 2
    between /= W
    eta = np.zeros(mean.shape)
    np.divide(between, var, out=eta, where=var > 0)
    return eta, mean, var
