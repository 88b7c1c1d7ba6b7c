"""numpy replay of the arithmetic of ps_contrast_* / predictive.PlanContrast: one add of a pair of fields, one
rounded operation per statement, so that the device's mean and every count can be compared bit for bit (M2 not:
the device contracts its last product into an fma, as sens_ref notes); and the weighted two-pass moments the
variance is checked against.  Shared by the CPU and GPU contrast tests."""
import numpy as np

import sens_ref


def new_state(shape, thresholds):
    """the accumulator of one output: moments of d = a - b, the count planes, the members' coverage rows"""
    k = len(thresholds)
    return {'thr': [float(t) for t in thresholds], 'W': 0, 'mean': np.zeros(shape), 'M2': np.zeros(shape),
            'pos': np.zeros(shape, dtype=np.int64), 'neg': np.zeros(shape, dtype=np.int64),
            'gain': np.zeros((k,) + tuple(shape), dtype=np.int64),
            'loss': np.zeros((k,) + tuple(shape), dtype=np.int64),
            'cells_a': [], 'cells_b': [], 'weights': []}


def add(state, a, b, w):
    """one member: fields a and b of the two plans, integer weight w.  d = a - b, then the statements of
    sens_ref.add (the step of ps_summary) on d; the counts; the member's row."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    w = int(w)
    d = a - b
    west = {'W': state['W'], 'mean': state['mean'], 'M2': state['M2'], 'C': np.zeros((0,) + d.shape)}
    sens_ref.add(west, d, [], w)
    state['mean'], state['M2'], state['W'] = west['mean'], west['M2'], west['W']
    state['pos'] += w * (d > 0)
    state['neg'] += w * (d < 0)
    na, nb = [], []
    for k, t in enumerate(state['thr']):
        state['gain'][k] += w * ((a >= t) & (b < t))
        state['loss'][k] += w * ((b >= t) & (a < t))
        na.append(int((a >= t).sum()))
        nb.append(int((b >= t).sum()))
    state['cells_a'].append(na)
    state['cells_b'].append(nb)
    state['weights'].append(w)
    return state


def planes(state):
    """the count planes in the device's order: pos, neg, gain_0, loss_0, gain_1, ..."""
    out = [state['pos'], state['neg']]
    for k in range(len(state['thr'])):
        out += [state['gain'][k], state['loss'][k]]
    return out


def two_pass(da, weights):
    """weighted mean and population variance of the fields da [member, ...]"""
    w = np.asarray(weights, dtype=np.float64).reshape((-1,) + (1,) * (np.ndim(da) - 1))
    da = np.asarray(da, dtype=np.float64)
    mean = (w * da).sum(0) / w.sum()
    return mean, (w * (da - mean) ** 2).sum(0) / w.sum()
