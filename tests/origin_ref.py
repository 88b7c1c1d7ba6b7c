"""The numpy restatement of the origin maps (include/parasitoid_hip.h, ps_origin_*; predictive.OriginMaps), statement
by statement, and a 40-digit mpmath version of l, E and the member rows with the bounds of DESIGN 7y.

fields: {lag: {model day of that lag's model: [N, N] float64}} -- the record values as ps_summary_add adds them, as
fetched from the host.  findings: checked probes (predictive.check_probes) with row, col, day.  hypotheses:
[(amount, lag), ...]."""
import math

import numpy as np

from parasitoids_amd.predictive import probe_loglik

EPS = 2.0 ** -53
NINF = -np.inf


def kernel_order(findings):
    """the findings that can give -inf ('found', 'count' with n > 0) first, each class in the order given"""
    hard = [o for o, f in enumerate(findings) if f['kind'] == 'found' or (f['kind'] == 'count' and f['n'] > 0)]
    return hard + [o for o in range(len(findings)) if o not in hard]


def shifted_plain(field, fr, fc):
    """G[r, c] = field[fr + R - r, fc + R - c], 0 where the source row or column leaves [0, N): what the finding at
    (fr, fc) sees of the centre release's field when the release is moved to (r, c); the indices written out"""
    N = field.shape[0]
    R = N // 2
    out = np.zeros((N, N), dtype=np.float64)
    for r in range(N):
        rs = fr + R - r
        if not 0 <= rs < N:
            continue
        for c in range(N):
            cs = fc + R - c
            if 0 <= cs < N:
                out[r, c] = field[rs, cs]
    return out


def shifted(field, fr, fc):
    """shifted_plain as one flipped slice copy: the candidates r0 .. r1 read the source rows fr + R - r1 .. fr + R - r0
    backwards, the columns likewise"""
    N = field.shape[0]
    R = N // 2
    out = np.zeros((N, N), dtype=np.float64)
    r0, r1 = max(0, fr + R - N + 1), min(N - 1, fr + R)
    c0, c1 = max(0, fc + R - N + 1), min(N - 1, fc + R)
    out[r0:r1 + 1, c0:c1 + 1] = field[fr + R - r1:fr + R - r0 + 1, fc + R - c1:fc + R - c0 + 1][::-1, ::-1]
    return out


def seen(findings, fields, lag):
    """per finding the plane of v under a release `lag` days after the first: zeros before the release"""
    out = []
    for f in findings:
        d = f['day'] - lag
        if d < 0:
            out.append(np.zeros_like(next(iter(fields[lag].values()))))
        else:
            out.append(shifted(fields[lag][d], f['row'], f['col']))
    return out


def loglik(findings, hypotheses, fields, log_prior=None):
    """[H, N, N] float64: l_h(s) through probe_loglik at mu = (rate * amount) * v, summed from 0.0 in the kernel's
    order; -inf at the cells the prior masks"""
    order = kernel_order(findings)
    planes = {lag: seen(findings, fields, lag) for lag in {g for _a, g in hypotheses}}
    out = []
    for amount, lag in hypotheses:
        V = planes[lag]
        N = V[0].shape[0]
        acc = np.zeros((N, N), dtype=np.float64)
        for o in order:
            f = findings[o]
            ra = f['rate'] * amount
            term = np.full((N, N), probe_loglik(f['kind'], ra, 0.0, f['n']), dtype=np.float64)
            for r, c in np.argwhere(V[o] != 0.0):
                term[r, c] = probe_loglik(f['kind'], ra, V[o][r, c], f['n'])
            acc = acc + term
        if log_prior is not None:
            acc = np.where(log_prior == NINF, NINF, acc)
        out.append(acc)
    return np.stack(out)


def loglik_mp(findings, hypotheses, fields, log_prior=None):
    """(l [H, N, N] object: mpf, or None where -inf;  parts [H, N, N] float64: the sum over the findings of
    |n log mu| + mu + lgamma(n + 1), what the bound of l scales with).  mu itself is the fp64 product
    fl(fl(rate * amount) * v): the inputs of the terms are the device's, the terms are exact."""
    import mpmath as mp
    mp.mp.dps = 40
    planes = {lag: seen(findings, fields, lag) for lag in {g for _a, g in hypotheses}}
    ls, ps = [], []
    for amount, lag in hypotheses:
        V = planes[lag]
        N = V[0].shape[0]
        l = np.empty((N, N), dtype=object)
        parts = np.zeros((N, N), dtype=np.float64)
        for r in range(N):
            for c in range(N):
                if log_prior is not None and log_prior[r, c] == NINF:
                    l[r, c] = None
                    continue
                acc, part = mp.mpf(0), 0.0
                for o, f in enumerate(findings):
                    mu = (f['rate'] * amount) * V[o][r, c]
                    if f['kind'] == 'none' or (f['kind'] == 'count' and f['n'] == 0):
                        acc -= mp.mpf(mu)
                        part += mu
                    elif mu == 0.0:
                        acc = None
                        break
                    elif f['kind'] == 'found':
                        t = mp.log(-mp.expm1(-mp.mpf(mu)))
                        acc += t
                        part += abs(float(t))
                    else:
                        m = mp.mpf(mu)
                        acc += f['n'] * mp.log(m) - m - mp.loggamma(f['n'] + 1)
                        part += abs(f['n'] * math.log(mu)) + mu + math.lgamma(f['n'] + 1)
                l[r, c] = acc
                parts[r, c] = part if acc is not None else 0.0
        ls.append(l)
        ps.append(parts)
    return np.stack(ls), np.stack(ps)


def loglik_parts(findings, hypotheses, fields):
    """parts [H, N, N] in float64, as loglik_mp returns them (0 where l is -inf)"""
    planes = {lag: seen(findings, fields, lag) for lag in {g for _a, g in hypotheses}}
    out = []
    for amount, lag in hypotheses:
        V = planes[lag]
        parts = np.zeros_like(V[0])
        dead = np.zeros(V[0].shape, dtype=bool)
        for o, f in enumerate(findings):
            mu = (f['rate'] * amount) * V[o]
            soft = f['kind'] == 'none' or (f['kind'] == 'count' and f['n'] == 0)
            with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
                if soft:
                    parts = parts + mu
                elif f['kind'] == 'found':
                    parts = parts + np.abs(np.log(-np.expm1(-mu)))
                else:
                    parts = parts + np.abs(f['n'] * np.log(mu)) + mu + math.lgamma(f['n'] + 1)
            if not soft:
                dead |= mu == 0.0
        out.append(np.where(dead, 0.0, parts))
    return np.stack(out)


def diff(got, want_mp):
    """|got - want| per entry, the difference taken in 40 digits: got float64, want mpf (1-D, same length)"""
    import mpmath as mp
    return np.array([abs(float(mp.mpf(float(g)) - t)) for g, t in zip(got, want_mp)], dtype=np.float64)


def finite_mask(l_mp):
    return np.vectorize(lambda v: v is not None, otypes=[bool])(l_mp)


def loglik_bound(nfind, parts):
    """|l_dev - l_mp| <= (O + 8) eps sum |parts|: per term a few roundings and one library call of <= 1..2 ulp on
    either side, O more for the sum"""
    return (nfind + 8) * EPS * parts


def lse_add(A, S, x, w):
    """the streaming update of (A, S) by a term of log-value x and mass w (arrays, elementwise), statement by
    statement: x = -inf nothing; A = -inf: (x, w); x <= A: S + w exp(x - A); else S exp(A - x) + w, A = x"""
    A, S = A.copy(), S.copy()
    w = np.broadcast_to(np.asarray(w, dtype=np.float64), A.shape)
    for i in np.ndindex(A.shape):
        xi = x[i]
        if xi == NINF:
            continue
        if A[i] == NINF:
            A[i], S[i] = xi, w[i]
        elif xi <= A[i]:
            S[i] = S[i] + w[i] * math.exp(xi - A[i])
        else:
            S[i] = S[i] * math.exp(A[i] - xi) + w[i]
            A[i] = xi
    return A, S


def accumulate(ls, weights):
    """(A, S) after the members' l planes [M][...] with integer weights, in order, from (-inf, 0)"""
    A = np.full(ls[0].shape, NINF)
    S = np.zeros(ls[0].shape)
    for l, w in zip(ls, weights):
        A, S = lse_add(A, S, l, float(w))
    return A, S


def merge(A, S, A2, S2):
    return lse_add(A, S, A2, S2)


def evidence(A, S, W):
    with np.errstate(divide='ignore', invalid='ignore'):
        E = A + np.log(S) - math.log(W)
    return np.where(A == NINF, NINF, E)


def evidence_mp(ls_mp, weights):
    """E = log(sum_m w_m exp(l_m) / W) per cell in 40 digits from the members' mp planes; None where every member
    is -inf"""
    import mpmath as mp
    W = sum(weights)
    out = np.empty(ls_mp[0].shape, dtype=object)
    for i in np.ndindex(out.shape):
        terms = [(l[i], w) for l, w in zip(ls_mp, weights) if l[i] is not None]
        if not terms:
            out[i] = None
            continue
        mx = max(t for t, _w in terms)
        out[i] = mx + mp.log(sum(w * mp.exp(t - mx) for t, w in terms) / W)
    return out


def evidence_bound(members, l_bound_max, E):
    """twice the largest l bound among the contributing members, plus (M + 8) eps (1 + |E|)"""
    return 2.0 * l_bound_max + (members + 8) * EPS * (1.0 + np.abs(E))


def rows(l, log_prior=None):
    """[H, 2]: (mx, sum) over the cells of x = l + log prior, summed in flat order"""
    out = []
    for lh in l:
        x = lh if log_prior is None else np.where(lh == NINF, NINF, lh + np.where(log_prior == NINF, 0.0, log_prior))
        mx = x.max()
        out.append((mx, 0.0 if mx == NINF else float(np.exp(x[x != NINF] - mx).sum())))
    return np.array(out)


def rows_mp(l_mp, log_prior=None):
    """per hypothesis (log of sum_s pi(s) exp l(s) in 40 digits or None, the number of finite cells)"""
    import mpmath as mp
    out = []
    for lh in l_mp:
        terms = [lh[i] + (0 if log_prior is None else mp.mpf(float(log_prior[i]))) for i in np.ndindex(lh.shape)
                 if lh[i] is not None]
        if not terms:
            out.append((None, 0))
            continue
        mx = max(terms)
        out.append((mx + mp.log(sum(mp.exp(t - mx) for t in terms)), len(terms)))
    return out


def row_bound(l_bound_max, cells, value):
    """|log(sum exp) error| <= the largest l bound (a shift of every exponent by at most that) plus (K + 8) eps
    (1 + |value|) for the K exponentials, their sum in any bracketing, the logarithm and the final sum"""
    return l_bound_max + (cells + 8) * EPS * (1.0 + abs(value))


def posterior_mp(E_mp, log_prior=None):
    """the posterior mass of every (hypothesis, cell) in 40 digits from E_mp (object array, None: -inf), as float64"""
    import mpmath as mp
    x = np.empty(E_mp.shape, dtype=object)
    for i in np.ndindex(E_mp.shape):
        lp = 0.0 if log_prior is None else float(log_prior[i[1:]])
        x[i] = None if E_mp[i] is None or lp == NINF else E_mp[i] + mp.mpf(lp)
    mx = max(v for v in x.ravel() if v is not None)
    w = np.array([mp.mpf(0) if v is None else mp.exp(v - mx) for v in x.ravel()], dtype=object)
    total = sum(w)
    return np.array([float(v / total) for v in w], dtype=np.float64).reshape(E_mp.shape)


def posterior_bound(e_bound_max, cells, P):
    """every exp(E - max) moves by at most 2 e_bound relatively (E and the maximum each by one), the normalising sum of
    K terms by as much plus K eps: |P_dev - P_mp| <= (4 e_bound + (K + 8) eps) P"""
    return (4.0 * e_bound_max + (cells + 8) * EPS) * P


def posterior(E, log_prior=None):
    x = E if log_prior is None else np.where(np.isnan(E + log_prior[None]), NINF, E + log_prior[None])
    p = np.exp(x - x.max())
    return p / p.sum()


def region(mass, level):
    """the smallest set of cells holding `level` of the mass: descending mass, ties by the smaller linear index"""
    flat = mass.ravel()
    order = sorted(range(flat.size), key=lambda i: (-flat[i], i))
    total, run = float(np.cumsum(flat[order])[-1]), np.cumsum(flat[order])
    out = np.zeros(flat.size, dtype=np.int8)
    for k, i in enumerate(order):
        out[i] = 1
        if run[k] >= level * total:
            break
    return out.reshape(mass.shape)


# ---------------------------------------------------------------- crafted inputs
def probe(row, col, day, kind, rate, n=None):
    return {'east': 0.0, 'north': 0.0, 'day': day, 'kind': kind, 'rate': rate, 'n': n, 'row': row, 'col': col}


def plume(N, row, col, sr, sc, total):
    """a Gaussian plume centred at (row, col), `total` wasps, cut to exact zero below 1e-8 as the records are"""
    r, c = np.mgrid[0:N, 0:N].astype(np.float64)
    g = np.exp(-0.5 * (((r - row) / sr) ** 2 + ((c - col) / sc) ** 2))
    g = g / g.sum() * total
    g[g < 1e-8] = 0.0
    return g


TWIN_N = 65
TWIN_K = 33
TWIN_DAYS = 3
TWIN_ORIGIN = (32 + 9, 32 - 7)       # 9 rows and -7 columns off the centre
TWIN_WEIGHTS = [1, 2, 1, 3, 1, 1, 2, 1]
TWIN_RATE = 1000.0                   # per unit of the release: the release at the centre has mass 1
TWIN_HYP = [(1.0, 0)]


def twin_stack(m):
    """member m of the twin experiment as a chain: (state coo, 3 day kernels coo) -- one wasp mass at the centre and
    Gaussian day kernels that drift and widen, another seed per member (synthetic.make_stack)"""
    from parasitoids_amd import synthetic
    state, kernels, _ = synthetic.make_stack(R=TWIN_N // 2, K=TWIN_K, ndays=TWIN_DAYS, seed=100 + m, sigma=(1.5, 3.0),
                                             shift=3.0)
    return state, kernels


def twin_members():
    """8 synthetic Gaussian-plume members over 3 days at N = 65 through the numpy oracle of the chain:
    {0: {day: field}} per member, day 0 the release"""
    from oracle import calcsol as OC
    out = []
    for m in range(8):
        state, kernels = twin_stack(m)
        ref = [state]
        OC.get_solutions(ref, [None] + kernels, list(range(TWIN_DAYS + 1)), TWIN_DAYS + 1, TWIN_N,
                         np.array([TWIN_K, TWIN_K]))
        out.append({0: {d: np.asarray(ref[d].todense()) for d in range(TWIN_DAYS + 1)}})
    return out


def twin_findings():
    """7 findings: 4 counts rounded from member 3's field translated to TWIN_ORIGIN, 3 'none'"""
    truth = twin_members()[3][0]
    dr, dc = TWIN_ORIGIN[0] - TWIN_N // 2, TWIN_ORIGIN[1] - TWIN_N // 2
    spots = [(1, -2, -1), (2, -3, -4), (2, -1, -2), (3, -5, -3)]     # (day, rows and columns off the known origin)
    out = []
    for d, a, b in spots:
        row, col = TWIN_ORIGIN[0] + a, TWIN_ORIGIN[1] + b
        v = truth[d][row - dr, col - dc]
        out.append(probe(row, col, d, 'count', TWIN_RATE, int(round(TWIN_RATE * v))))
    for d, row, col in [(1, 8, 50), (2, 55, 55), (3, 20, 10)]:
        out.append(probe(row, col, d, 'none', TWIN_RATE))
    return out
