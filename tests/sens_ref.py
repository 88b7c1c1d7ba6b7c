"""numpy replay of the arithmetic of ps_sens_* / predictive.SensitivityMaps: one add and the finalize, one
rounded operation per statement, so that the device's mean, co-moments, explained share and dominant index can
be compared bit for bit; and the weighted two-pass moments the tolerances are checked against.  Shared by the
CPU and GPU sensitivity tests."""
import numpy as np


def new_state(shape, nparam):
    return {'W': 0, 'mean': np.zeros(shape), 'M2': np.zeros(shape), 'C': np.zeros((nparam,) + tuple(shape))}


def add(state, v, e, w):
    """one member: field v, deviations e[nparam] of its scalars from their updated means, integer weight w.
    mean and every C_i follow the device bit for bit; M2 does not (the device contracts its last product into
    an fma, as ps_summary does)."""
    v = np.asarray(v, dtype=np.float64)
    w = float(int(w))
    Wn = float(state['W'] + int(w))
    mean = state['mean']
    d = v - mean
    ch = d != 0.0
    t = d * w
    t = t / Wn
    mean1 = np.where(ch, mean + t, mean)
    wd = w * d
    r = v - mean1
    state['M2'] = np.where(ch, state['M2'] + wd * r, state['M2'])
    for i in range(state['C'].shape[0]):
        prod = wd * float(e[i])
        state['C'][i] = np.where(ch, state['C'][i] + prod, state['C'][i])
    state['mean'] = mean1
    state['W'] += int(w)
    return state


def finalize(cov, var, F, isd):
    """(expl, dom) from the fetched maps cov[nparam] = C_i / W and var = M2 / W, the factor F[nparam, rank] and
    isd[nparam]: expl = sum_k (sum_i F_ik c_i)^2 / var, 0 where var == 0; dom = the lowest i that maximises
    (c_i isd_i)^2 by a strict >, -1 where var == 0 or every square is 0"""
    cov = np.asarray(cov, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    F = np.asarray(F, dtype=np.float64)
    nparam, rank = F.shape
    s = np.zeros(var.shape)
    for k in range(rank):
        u = np.zeros(var.shape)
        for i in range(nparam):
            prod = F[i, k] * cov[i]
            u = u + prod
        sq = u * u
        s = s + sq
    live = var != 0.0
    expl = np.zeros(var.shape)
    np.divide(s, var, out=expl, where=live)
    best = np.zeros(var.shape)
    dom = np.full(var.shape, -1, dtype=np.int8)
    for i in range(nparam):
        t = cov[i] * float(isd[i])
        t2 = t * t
        up = live & (t2 > best)
        dom[up] = i
        best = np.where(up, t2, best)
    return expl, dom


def two_pass(fields, thetas, weights):
    """weighted mean [*shape], variance [*shape], covariance [nparam, *shape] with every scalar, and the
    scalars' covariance matrix, from the dense fields [member, *shape] and scalars [member, nparam]"""
    w = np.asarray(weights, dtype=np.float64)
    X = np.asarray(fields, dtype=np.float64)
    T = np.asarray(thetas, dtype=np.float64)
    W = w.sum()
    mean = np.tensordot(w, X, axes=1) / W
    tm = w @ T / W
    dX = X - mean[None]
    dT = T - tm[None]
    var = np.tensordot(w, dX ** 2, axes=1) / W
    cov = np.array([np.tensordot(w * dT[:, i], dX, axes=1) / W for i in range(T.shape[1])])
    return mean, var, cov, (dT * w[:, None]).T @ dT / W
