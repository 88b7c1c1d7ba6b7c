"""numpy replay of the arithmetic of ps_rank_* / predictive.PlanRanking: one add of the P plans' fields of one
member, one rounded operation per statement, so that the device's regret means, every count plane and every
coverage row can be compared bit for bit (M2 not: the device contracts its last product into an fma, as sens_ref
notes); and the weighted two-pass moments the variance is checked against.  Shared by the CPU and GPU ranking
tests."""
import numpy as np

import sens_ref


def new_state(shape, nplan, thresholds):
    """the accumulator of one output: per plan the moments of its regret and its best plane, per threshold the
    sole planes, any and all, and the members' coverage rows"""
    k = len(thresholds)
    shape = tuple(shape)
    return {'thr': [float(t) for t in thresholds], 'P': int(nplan), 'W': 0,
            'mean': np.zeros((nplan,) + shape), 'M2': np.zeros((nplan,) + shape),
            'best': np.zeros((nplan,) + shape, dtype=np.int64),
            'sole': np.zeros((k, nplan) + shape, dtype=np.int64),
            'any': np.zeros((k,) + shape, dtype=np.int64), 'all': np.zeros((k,) + shape, dtype=np.int64),
            'cells': [], 'weights': []}


def add(state, fields, w):
    """one member: fields[j] of plan j, integer weight w.  m = max_j a_j; best_j where a_j == m and no other plan
    holds m; r_j = m - a_j, then the statements of sens_ref.add (the step of ps_summary) on r_j; the threshold
    counts; the member's row [plan][threshold]."""
    a = np.array([np.asarray(f, dtype=np.float64) for f in fields])
    P = state['P']
    assert a.shape[0] == P
    w = int(w)
    m = a.max(axis=0)
    nmax = (a == m).sum(axis=0)
    for j in range(P):
        state['best'][j] += w * ((a[j] == m) & (nmax == 1))
        r = m - a[j]
        west = {'W': state['W'], 'mean': state['mean'][j], 'M2': state['M2'][j], 'C': np.zeros((0,) + r.shape)}
        sens_ref.add(west, r, [], w)
        state['mean'][j], state['M2'][j] = west['mean'], west['M2']
    row = [[0] * len(state['thr']) for _ in range(P)]
    for k, t in enumerate(state['thr']):
        n = (a >= t).sum(axis=0)
        for j in range(P):
            state['sole'][k, j] += w * ((a[j] >= t) & (n == 1))
            row[j][k] = int((a[j] >= t).sum())
        state['any'][k] += w * (n >= 1)
        state['all'][k] += w * (n == P)
    state['W'] += w
    state['cells'].append(row)
    state['weights'].append(w)
    return state


def planes(state):
    """the count planes in the device's order: best_0 .. best_{P-1}, then per k sole_k0 .. sole_k,P-1, any_k, all_k"""
    out = [state['best'][j] for j in range(state['P'])]
    for k in range(len(state['thr'])):
        out += [state['sole'][k, j] for j in range(state['P'])] + [state['any'][k], state['all'][k]]
    return out


def rows(state):
    """[members, P, nthr] int64: the members' coverage rows in add order"""
    return np.array(state['cells'], dtype=np.int64).reshape(len(state['cells']), state['P'], len(state['thr']))


def regrets(fields):
    """[member, plan, ...]: max over the plans minus each plan, from the fields [member][plan]"""
    a = np.asarray(fields, dtype=np.float64)
    return a.max(axis=1, keepdims=True) - a


def two_pass(da, weights):
    """weighted mean and population variance of the fields da [member, ...]"""
    w = np.asarray(weights, dtype=np.float64).reshape((-1,) + (1,) * (np.ndim(da) - 1))
    da = np.asarray(da, dtype=np.float64)
    mean = (w * da).sum(0) / w.sum()
    return mean, (w * (da - mean) ** 2).sum(0) / w.sum()
