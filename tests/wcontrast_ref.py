"""ps_wcontrast restated in numpy, sharing no code with the package: the scale rule of the log-weights, one add of one
scenario with one rounded operation per line, the merge, and the plain two-pass definitions with normalised weights.
Shared by test_wcontrast_cpu.py and test_wcontrast_gpu.py.

One add of a member (a, b) with rescale r and weight om > 0 into (W, mean, M2, S_0 .. S_{P-1}), the statements of the
header in their order:
    W = W * r;  W = W + om
    d = a - b
    M2 = M2 * r;  S_p = S_p * r
    e = d - mean;  e != 0:  mean = mean + (e * om) / W;  M2 = fma(om * e, d - mean, M2)
    d > 0: S_pos = S_pos + om;  d < 0: S_neg = S_neg + om
    a >= t_k and b < t_k: S_gain_k = S_gain_k + om;  b >= t_k and a < t_k: S_loss_k = S_loss_k + om
The M2 step is crafted_fields.fma: what contraction makes of sum_update's `m2 += w * d * (v - m)`, as
crafted_fields.welford(fused=True) has it for integer weights.  om == 0 leaves the scenario untouched.

The four weight sets of the tests (LAM, one log-weight per member of crafted_plans.pair_members, run lengths
crafted_plans.WEIGHTS): `flat` all 0; `swing` raises the reference twice and lets tiny weights follow; `dead` starts
late and skips three members; `under` skips a member whose weight underflows and then wipes what came before with
r = exp(-800) = 0.

Against the exact rational moments of d, with the doubles om and r taken as exact Fractions (a member's final
weight is its om times every later r), the largest over every cell of pair_members(N), every entry, N = 65 and 129,
measured by test_wcontrast_cpu.py, which asserts them with a margin of 2.  The units are those of
crafted_fields.moment_errors with the weights the members had when they were added (their om), over the members
the scenario took: a later rescale shrinks what is held, but not the rounding error the mean already carries, and
with r = 0 the mean that stays behind is the starting point of the next step, so the error is one of the values that
passed through, not of those that still weigh.  Both units are floored at 2^-1075 (crafted_plans.FLOOR).
    scenario   mean, units of 2^-53 max_m |d_m|    M2, units of 2^-53 sum_m om_m d_m^2
    flat       0.5427                               2.0993
    swing      0.0001                               0.0001
    dead       0.8852                               1.2646
    under      0.6409                               0.2747
each rounded up to four decimals (swing: both below 5e-5 -- its last heavy member outweighs the others by 170 orders
of magnitude, and the step that takes it lands on its value exactly).
(MEAN_ERR, M2_ERR below.)
"""
import math
from fractions import Fraction
from functools import lru_cache

import numpy as np

import crafted_fields as CF
import crafted_plans as CP

NAMES = ('flat', 'swing', 'dead', 'under')
INF = math.inf
LAM = {'flat': (0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
       'swing': (0.0, 0.0, 300.0, -300.0, 700.5, 10.0),
       'dead': (-INF, 0.0, -INF, 0.0, 0.0, -INF),
       'under': (0.0, 0.0, -800.0, 0.0, 800.0, 0.0)}
MEAN_ERR = {'flat': 0.5427, 'swing': 0.0001, 'dead': 0.8852, 'under': 0.6409}
M2_ERR = {'flat': 2.0993, 'swing': 0.0001, 'dead': 1.2646, 'under': 0.2747}


def member_lams(names=NAMES):
    """per member the log-weights of the scenarios `names`"""
    return [[LAM[n][m] for n in names] for m in range(len(CP.WEIGHTS))]


# ---- the scale rule -------------------------------------------------------------------------------------------------

def scale(ref, lam, weight):
    """one scenario: (r, om, ref') for a member of log-weight lam and run length weight, ref the largest log-weight so
    far (-inf while empty).  ref moves only if om > 0"""
    w = float(weight)
    if lam == -INF:
        return 1.0, 0.0, ref
    if ref == -INF:
        return 1.0, w, lam
    if lam > ref:
        return math.exp(ref - lam), w, lam
    om = w * math.exp(lam - ref)
    return 1.0, om, ref


def schedule(lams, weights):
    """the (r, om) of every member of one scenario in order, and the final ref"""
    ref, out = -INF, []
    for lam, w in zip(lams, weights):
        r, om, new = scale(ref, lam, w)
        out.append((r, om))
        if om > 0.0:
            ref = new
    return out, ref


def merge_scale(ref_a, ref_b):
    top = max(ref_a, ref_b)
    if top == -INF:
        return 1.0, 1.0, top
    return math.exp(ref_a - top), math.exp(ref_b - top), top


# ---- one scenario ---------------------------------------------------------------------------------------------------

def new(n, nthr):
    return {'W': 0.0, 'members': 0, 'skipped': 0, 'mean': np.zeros(n), 'M2': np.zeros(n),
            'S': [np.zeros(n) for _ in range(2 + 2 * nthr)]}


def add(st, a, b, r, om, thr):
    """the statements of the module docstring, one rounded operation per line"""
    if not om > 0.0:
        st['skipped'] += 1
        return
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        W = st['W'] * r
        W = W + om
        d = a - b
        q = st['M2'] * r
        S = [s * r for s in st['S']]
        e = d - st['mean']
        step = e * om
        step = step / W
        mean = np.where(e == 0.0, st['mean'], st['mean'] + step)
        x, y = om * e, d - mean
        for i in np.flatnonzero(e != 0.0):
            q[i] = CF.fma(float(x[i]), float(y[i]), float(q[i]))
        S[0] = np.where(d > 0.0, S[0] + om, S[0])
        S[1] = np.where(d < 0.0, S[1] + om, S[1])
        for k, t in enumerate(thr):
            S[2 + 2 * k] = np.where((a >= t) & (b < t), S[2 + 2 * k] + om, S[2 + 2 * k])
            S[3 + 2 * k] = np.where((b >= t) & (a < t), S[3 + 2 * k] + om, S[3 + 2 * k])
    st.update(W=W, mean=mean, M2=q, S=S)
    st['members'] += 1


def merge(dst, src, ra, rb):
    """dst += src by Chan, Golub & LeVeque with the expressions of k_wsum_merge as contraction leaves them:
        Wa = Wa * ra;  Wb = Wb * rb;  W = Wa + Wb;  e = mean_b - mean_a
        mean = fma(e, Wb / W, mean_a);  M2 = fma(e * e, (Wa * Wb) / W, fma(M2_a, ra, M2_b * rb));  S = fma(S_a, ra, S_b * rb)
    an empty src adds its skipped count alone, an empty dst becomes a copy"""
    if src['W'] == 0.0:
        dst['skipped'] += src['skipped']
        return
    if dst['W'] == 0.0:
        dst.update(W=src['W'], mean=src['mean'].copy(), M2=src['M2'].copy(), S=[s.copy() for s in src['S']])
    else:
        Wa, Wb = dst['W'] * ra, src['W'] * rb
        W = Wa + Wb
        c1, c2 = Wb / W, Wa * Wb / W
        with np.errstate(over='ignore', invalid='ignore', under='ignore'):
            e = src['mean'] - dst['mean']
            ee, qb = e * e, src['M2'] * rb
            n = e.size
            mean = np.array([CF.fma(float(e[i]), c1, float(dst['mean'][i])) for i in range(n)])
            q = np.array([CF.fma(float(ee[i]), c2, CF.fma(float(dst['M2'][i]), ra, float(qb[i]))) for i in range(n)])
            S = [np.array([CF.fma(float(sa[i]), ra, float(sb[i] * rb)) for i in range(n)])
                 for sa, sb in zip(dst['S'], src['S'])]
        dst.update(W=W, mean=mean, M2=q, S=S)
    dst['members'] += src['members']
    dst['skipped'] += src['skipped']


def fetch(st, what):
    """what ps_wcontrast_fetch returns: 0 mean, 1 M2 / W, 2 + p min(S_p / W, 1)"""
    with np.errstate(over='ignore', invalid='ignore'):
        if what == 0:
            return st['mean']
        if what == 1:
            return st['M2'] / st['W']
        p = st['S'][what - 2] / st['W']
        return np.where(p < 1.0, p, 1.0)


# ---- the plain definitions ------------------------------------------------------------------------------------------

def normalised(lams, weights):
    """omega_m = w_m exp(lam_m - max lam) / sum: the weights of one scenario, summing to 1"""
    lam = np.asarray(lams, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    top = lam[np.isfinite(lam)].max()
    om = w * np.exp(lam - top)
    return om / om.sum()


def two_pass(A, B, omega, thr):
    """A, B [M, ...], omega [M] summing to 1 -> dict(mean, var, pos, neg, gain [K], loss [K]), two passes"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    om = np.asarray(omega, dtype=np.float64).reshape((-1,) + (1,) * (A.ndim - 1))
    D = A - B
    with np.errstate(over='ignore', invalid='ignore'):
        mean = (om * D).sum(0)
        var = (om * (D - mean) ** 2).sum(0)
    return {'mean': mean, 'var': var, 'pos': (om * (D > 0)).sum(0), 'neg': (om * (D < 0)).sum(0),
            'gain': [(om * ((A >= t) & (B < t))).sum(0) for t in thr],
            'loss': [(om * ((B >= t) & (A < t))).sum(0) for t in thr]}


# ---- the crafted pairs under the four weight sets -------------------------------------------------------------------

@lru_cache(maxsize=None)
def reference(N):
    """per entry e of the profiles and scenario name: the state after the six pair_members(N) in order, thresholds
    THR4 (a handle of fewer thresholds holds the first planes, one of fewer scenarios the first names), and
    'sched': per scenario (the (r, om) of every member, the final ref)"""
    mem = CP.pair_members(N)
    sched = {n: schedule(LAM[n], CP.WEIGHTS) for n in NAMES}
    out = []
    for e in range(CP.NENTRY):
        ent = {}
        vals = [CP.values(m, e) for m in mem]
        for n in NAMES:
            st = new(N * N, len(CP.THR4))
            for (a, b), (r, om) in zip(vals, sched[n][0]):
                add(st, a, b, r, om, CP.THR4)
            ent[n] = st
        ent['D'] = np.array([a - b for a, b in vals])
        out.append(ent)
    return out, sched


def final_weights(steps):
    """the exact weight every member ends with: its om times every later r, as Fractions"""
    out = []
    for m, (_r, om) in enumerate(steps):
        w = Fraction(om)
        for r2, om2 in steps[m + 1:]:
            if om2 > 0.0:
                w *= Fraction(r2)
        out.append(w)
    return out


def exact_errors(st, D, steps):
    """the distance of (mean, M2) from the exact rational moments of the columns of D [M, n] under final_weights, in
    the units of the module docstring, at one cell of every distinct column -> (mean error, M2 error)"""
    wf = final_weights(steps)
    W = sum(wf)
    taken = [m for m, (_r, om) in enumerate(steps) if om > 0.0]
    _u, at = np.unique(D, axis=1, return_index=True)
    worst_m = worst_q = Fraction(0)
    for i in at:
        col = [Fraction(float(D[m, i])) for m in range(D.shape[0])]
        if not any(col[m] for m in taken):
            assert st['mean'][i] == 0 and st['M2'][i] == 0, i
            continue
        mean = sum(wf[m] * col[m] for m in taken) / W
        M2 = sum(wf[m] * (col[m] - mean) ** 2 for m in taken)
        um = max(Fraction(max(abs(col[m]) for m in taken), 2 ** 53), CP.FLOOR)
        uq = Fraction(sum(Fraction(steps[m][1]) * col[m] ** 2 for m in taken), 2 ** 53)
        worst_m = max(worst_m, abs(Fraction(float(st['mean'][i])) - mean) / um)
        q = float(st['M2'][i])
        if not math.isfinite(q):
            assert uq * 2 ** 53 >= 2 ** 1023, (i, q)
            continue
        worst_q = max(worst_q, abs(Fraction(q) - M2) / max(uq, CP.FLOOR))
    return float(worst_m), float(worst_q)
