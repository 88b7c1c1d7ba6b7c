"""The numpy restatement of the origin maps over known releases in the background (include/parasitoid_hip.h,
ps_origin_set_known / ps_origin_background; predictive.OriginMaps with known=), statement by statement from the
pieces of origin_ref, and its 40-digit mpmath version with the bounds of DESIGN 7y, unchanged.

fields: {lag: {model day of that lag's model: [N, N] float64}} as in origin_ref, holding every lag of the hypotheses
and of the known releases.  known: [dict(drow, dcol, amount, lag), ...] -- the cell offsets of check_sites."""
import math

import numpy as np

import origin_ref as OR
from parasitoids_amd.predictive import probe_loglik

NINF = -np.inf


def known(drow, dcol, amount, lag=0):
    return {'drow': int(drow), 'dcol': int(dcol), 'amount': float(amount), 'lag': int(lag)}


def background(findings, knowns, fields):
    """[O] float64 in the order given: bg_o = sum over k in index order, from +0.0, of fl(fl(rate_o * amount_k) * v_k);
    v_k the known lag's field of day d_o - lag_k at (row_o - drow_k, col_o - dcol_k), 0 where either axis leaves
    [0, N) and 0 before that release.  The numpy loop the device matches bit for bit."""
    out = np.zeros(len(findings), dtype=np.float64)
    for o, f in enumerate(findings):
        s = np.float64(0.0)
        for k in knowns:
            d = f['day'] - k['lag']
            v = np.float64(0.0)
            if d >= 0:
                field = fields[k['lag']][d]
                N = field.shape[0]
                rs, cs = f['row'] - k['drow'], f['col'] - k['dcol']
                if 0 <= rs < N and 0 <= cs < N:
                    v = np.float64(field[rs, cs])
            rak = np.float64(f['rate']) * np.float64(k['amount'])
            term = rak * v
            s = s + term
        out[o] = s
    return out


def term_at(f, mu):
    """origin_term: one finding's term at mu >= 0"""
    return probe_loglik(f['kind'], 1.0, float(mu), f['n'])


def null_row(findings, bg):
    """l0: the terms at mu = bg in the kernel's order, from +0.0"""
    s = 0.0
    for o in OR.kernel_order(findings):
        s = s + term_at(findings[o], bg[o])
    return s


def loglik(findings, hypotheses, fields, bg, log_prior=None):
    """[H, N, N] float64: l_h(s) with t = fl(ra * v), mu = fl(bg_o + t), summed from 0.0 in the kernel's order; -inf at
    the cells the prior masks"""
    order = OR.kernel_order(findings)
    planes = {lag: OR.seen(findings, fields, lag) for lag in {g for _a, g in hypotheses}}
    out = []
    for amount, lag in hypotheses:
        V = planes[lag]
        N = V[0].shape[0]
        acc = np.zeros((N, N), dtype=np.float64)
        for o in order:
            f = findings[o]
            ra = f['rate'] * amount
            term = np.full((N, N), term_at(f, bg[o]), dtype=np.float64)     # t = 0: mu = bg exactly
            for r, c in np.argwhere(V[o] != 0.0):
                t = ra * V[o][r, c]
                mu = bg[o] + t
                term[r, c] = term_at(f, mu)
            acc = acc + term
        if log_prior is not None:
            acc = np.where(log_prior == NINF, NINF, acc)
        out.append(acc)
    return np.stack(out)


def _terms_mp(findings, mus):
    """(the exact sum of the terms at the fp64 numbers mus or None for -inf, what the bound scales with)"""
    import mpmath as mp
    acc, part = mp.mpf(0), 0.0
    for f, mu in zip(findings, mus):
        mu = float(mu)
        if f['kind'] == 'none' or (f['kind'] == 'count' and f['n'] == 0):
            acc -= mp.mpf(mu)
            part += mu
        elif mu == 0.0:
            return None, 0.0
        elif f['kind'] == 'found':
            t = mp.log(-mp.expm1(-mp.mpf(mu)))
            acc += t
            part += abs(float(t))
        else:
            m = mp.mpf(mu)
            acc += f['n'] * mp.log(m) - m - mp.loggamma(f['n'] + 1)
            part += abs(f['n'] * math.log(mu)) + mu + math.lgamma(f['n'] + 1)
    return acc, part


def null_row_mp(findings, bg):
    """(l0 in 40 digits or None, parts): the inputs are the device's fp64 bg, the terms are exact"""
    import mpmath as mp
    mp.mp.dps = 40
    return _terms_mp(findings, bg)


def loglik_mp(findings, hypotheses, fields, bg, log_prior=None):
    """as origin_ref.loglik_mp with mu = fl(bg_o + fl(fl(rate * amount) * v)) -- the fp64 number the device forms; a
    cell whose shifted reads are all 0 shares the null row's value, computed once"""
    import mpmath as mp
    mp.mp.dps = 40
    planes = {lag: OR.seen(findings, fields, lag) for lag in {g for _a, g in hypotheses}}
    null = _terms_mp(findings, bg)
    ls, ps = [], []
    for amount, lag in hypotheses:
        V = planes[lag]
        N = V[0].shape[0]
        l = np.empty((N, N), dtype=object)
        parts = np.zeros((N, N), dtype=np.float64)
        touched = np.zeros((N, N), dtype=bool)
        for v in V:
            touched |= v != 0.0
        for r in range(N):
            for c in range(N):
                if log_prior is not None and log_prior[r, c] == NINF:
                    l[r, c] = None
                    continue
                if not touched[r, c]:
                    l[r, c], parts[r, c] = null
                    continue
                mus = []
                for o, f in enumerate(findings):
                    t = (f['rate'] * amount) * V[o][r, c]
                    mus.append(bg[o] + t)
                l[r, c], parts[r, c] = _terms_mp(findings, mus)
        ls.append(l)
        ps.append(parts)
    return np.stack(ls), np.stack(ps)


def loglik_parts(findings, hypotheses, fields, bg):
    """parts [H, N, N] in float64, as loglik_mp returns them (0 where l is -inf)"""
    planes = {lag: OR.seen(findings, fields, lag) for lag in {g for _a, g in hypotheses}}
    out = []
    for amount, lag in hypotheses:
        V = planes[lag]
        parts = np.zeros_like(V[0])
        dead = np.zeros(V[0].shape, dtype=bool)
        for o, f in enumerate(findings):
            t = (f['rate'] * amount) * V[o]
            mu = bg[o] + t
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


def untouched(findings, hypotheses, fields):
    """[H, N, N] bool: the candidate cells whose shifted reads are all 0 -- there l_h(s) == l0 bit for bit"""
    out = []
    for _amount, lag in hypotheses:
        t = np.zeros_like(next(iter(fields[lag].values())), dtype=bool)
        for v in OR.seen(findings, fields, lag):
            t |= v != 0.0
        out.append(~t)
    return np.stack(out)


def log_mean_exp(values, weights):
    """log(sum w exp(x) / sum w)"""
    x, w = np.asarray(values, dtype=np.float64), np.asarray(weights, dtype=np.float64)
    mx = x.max()
    return -np.inf if mx == NINF else float(mx + np.log((w * np.exp(x - mx)).sum() / w.sum()))


# ---------------------------------------------------------------- the twin experiment with our release known
TWIN_SECOND = 0.5                                      # the second source's amount, at origin_ref.TWIN_ORIGIN
TWIN_NEAR = [(1, 1, 2), (2, 3, 4), (3, 4, 6)]          # (day, rows and columns off the centre): traps near our release
TWIN_AMOUNTS = [0.25, 0.5, 1.0]
TWIN_KNOWN = [known(0, 0, 1.0, 0)]


def twin_hypotheses():
    return [(a, 0) for a in TWIN_AMOUNTS]


def twin_findings(second=True, members=None):
    """round(1000 (ours + 0.5 shifted)) at the four spots of origin_ref.twin_findings and at three cells near our
    release, and the three 'none' of origin_ref; second=False: the same traps with our release alone"""
    truth = (members or OR.twin_members())[3][0]
    R = OR.TWIN_N // 2
    dr, dc = OR.TWIN_ORIGIN[0] - R, OR.TWIN_ORIGIN[1] - R

    def count(d, row, col):
        ours = truth[d][row, col]
        rs, cs = row - dr, col - dc
        moved = truth[d][rs, cs] if 0 <= rs < OR.TWIN_N and 0 <= cs < OR.TWIN_N else 0.0
        return int(round(OR.TWIN_RATE * (ours + (TWIN_SECOND * moved if second else 0.0))))
    spots = [(1, -2, -1), (2, -3, -4), (2, -1, -2), (3, -5, -3)]
    out = []
    for d, a, b in spots:
        row, col = OR.TWIN_ORIGIN[0] + a, OR.TWIN_ORIGIN[1] + b
        out.append(OR.probe(row, col, d, 'count', OR.TWIN_RATE, count(d, row, col)))
    for d, a, b in TWIN_NEAR:
        out.append(OR.probe(R + a, R + b, d, 'count', OR.TWIN_RATE, count(d, R + a, R + b)))
    for d, row, col in [(1, 8, 50), (2, 55, 55), (3, 20, 10)]:
        out.append(OR.probe(row, col, d, 'none', OR.TWIN_RATE))
    return out


def twin_summary(ls, l0s, weights, log_prior=None):
    """from the members' l [M][H, N, N] and l0 [M]: (posterior [H, N, N], log Bayes factor second : ours alone) by the
    host functions of predictive"""
    from parasitoids_amd import predictive as PR
    A, S = OR.accumulate(ls, weights)
    E = PR.origin_log_evidence(A, S, sum(weights))
    P = PR.origin_posterior(E, log_prior)
    lbf = PR.origin_log_evidence_second(E, log_prior) - PR.origin_log_mean_exp(l0s, weights)
    return P, lbf
