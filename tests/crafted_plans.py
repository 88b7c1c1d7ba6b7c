"""Crafted plans for the paired accumulators (ps_rank, ps_contrast) and the sources on the way to them (ps_project,
ps_sites), on top of crafted_fields.py: P fields per member that sit on every comparison the kernels make, and
references that share nothing with the library.  Shared by test_crafted_plans_cpu.py and test_crafted_plans_gpu.py.

Feeding.  A projection with nin = nout = S and the identity matrix gives Y_e = +0.0 + 1.0 * v_e = v_e bit for bit, and
a release plan with the one site (0, 0, 1.0) does the same, so plan j of a member is one crafted field injected into
the solver and applied under a slot profile; the tests read every Y_e back and require history(field, profile) before
anything else is compared.

A *member* is (name, fields [P, N, N], profile name, weight, negval).  negval = 0 keeps the values far below the
package's 1e-8 that the tie blocks hold; the package's own negval lets the 'cut' profile cut.  The weights (WEIGHTS)
sum to 16, so the variance M2 / W that the library returns is M2 with another exponent: equal variances are equal M2,
and M2 comes back from a fetched variance without a rounding.  The first two members are the same and the first has
weight 1 (v * 1 / 1 is v, v * 3 / 3 need not be): after them the mean is the value bit for bit.  The last is zero.

Slots.  A handle of S slots holds, in slot s, entry entry_of(s) = (s + s // 6) % 5 of the member's 5-entry profile.
For S = 5 that is s itself.  Plain s % 5 would give slot 20 of the six-plan case the plane of slot 0 -- the very slot
a second chunk written to `slot - chunk` would hit -- so the entry moves on by one more with every six slots:
neighbouring slots never share an entry, nor do the slots s and s - chunk for any chunk of a ranking add (16, 18, 20,
24, 28), and a reference computed once for the five entries serves every S.

Where double itself ends.  Ties at 1e300 have regrets (one ulp of 1e300 and more) whose square is beyond the largest
double: M2 is +inf there in the references and on the device alike, compared bit for bit like any other value, and
left out of the distance from the exact moments (moment_errors requires sum w v^2 >= 2^1023 wherever it meets an
infinity).  Ties at 1e-300 and at subnormals have squares below the smallest subnormal: there no double has digits
left, so both units of crafted_fields are floored at 2^-1075, half the smallest subnormal, the absolute error of one
rounding down there.

The restatements (welford / merge_fused of crafted_fields on the regrets and differences) against the exact rational
moments, the largest over plan_members at P = 2 .. 8 and pair_members, every entry, every plan, the merges in both
orders, at both sizes (measured by test_crafted_plans_cpu.py, which asserts them with a margin of 2):
    mean, in units of 2^-53 * max_m |v_m|:    2.0000 (MEAN_ERR; at a subnormal mean, one of its ulps)
    M2, in units of 2^-53 * sum_m w_m v_m^2:  2.6256 (M2_ERR)
"""
import math
from fractions import Fraction
from functools import lru_cache

import numpy as np

import crafted_fields as CF

MEAN_ERR = 2.0
M2_ERR = 2.6256

NEGVAL = CF.NEGVAL
SIZES = CF.SIZES
PLANS = tuple(range(2, 9))
NENTRY = CF.NSLOT
THR4 = CF.THR + (1e3,)                  # the thresholds of a handle with nthr = k are THR4[:k]
WEIGHTS = (1, 3, 3, 3, 3, 3)
HALF = 3                                # the merged handles: members 0 .. 2 and 3 .. 5
SUBNORMAL = 1000 * 5e-324
FLOOR = Fraction(1, 2 ** 1075)
SHORT = 12                              # cells of the short block
HOT = CF.HOT
HOT_SPAN = 2 * HOT + HOT // 7 + 2
THR_BLOCKS = tuple((k, up) for k in range(3) for up in (0, 1)) + ((3, 0),)      # (threshold of THR4, at it / just above)

# name, rotation of the plans (and k of 1e-300 * 2^k and of the HOT regrets), profile, negval, the tail block whole
_SEQ = (('base', 0, 'sum', 0.0, True), ('base again', 0, 'sum', 0.0, True), ('rot1', 1, 'cut', NEGVAL, True),
        ('rot2', 2, 'prob', 0.0, False), ('rot3', 3, 'rising', NEGVAL, True), ('zero', None, 'falling', NEGVAL, True))


def entry_of(s):
    return (s + s // 6) % 5


def slot_profile(profile, S):
    """the (stat_scale, post_scale) of a handle of S slots under a 5-entry profile"""
    stat, post = CF.PROFILES[profile]
    return tuple(stat[entry_of(s)] for s in range(S)), tuple(post[entry_of(s)] for s in range(S))


def rank_chunk(P):
    """the slots of one launch of a ranking add: 1152 bytes of descriptors of 8 P + 8 bytes, 32 at the most"""
    return min(32, 1152 // (8 * P + 8))


# ---- the plan zoo ---------------------------------------------------------------------------------------------------

def tie_m(k):
    return (25.0, 1e300, 1e-300 * 2.0 ** k, SUBNORMAL)


def tie_block(P, m, shift, masks=None):
    """[P, cases]: case `mask` has the plans of the subset at m, plan j outside it at nextafter(m, 0), m / 2 or 0"""
    masks = range(1, 2 ** P) if masks is None else masks
    rest = (math.nextafter(m, 0.0), m / 2, 0.0)
    return np.array([[m if mask >> j & 1 else rest[(2 * j + mask + shift) % 3] for mask in masks] for j in range(P)])


def thr_block(P, t, up, masks=None):
    """[P, cases]: the plans of the subset at t (up: at nextafter(t, inf)), the others at nextafter(t, 0)"""
    masks = range(2 ** P) if masks is None else masks
    hi, lo = (math.nextafter(t, math.inf) if up else float(t)), math.nextafter(t, 0.0)
    return np.array([[hi if mask >> j & 1 else lo for mask in masks] for j in range(P)])


def short_block(P):
    """SHORT cases: six ties at 25 and six subsets at the threshold 10; the last one is plan P - 1 alone at 10"""
    full = 2 ** P - 1
    return np.hstack([tie_block(P, 25.0, 0, (1, 2, 3, 1, full, 2 ** (P - 1))),
                      thr_block(P, 10.0, False, (0, 1, full, 2, 3, 2 ** (P - 1)))])


@lru_cache(maxsize=None)
def layout(N, P):
    """-> dict: the first flat cell of every block.  Every block starts at an odd cell, so the two cells 2i, 2i + 1 a
    thread owns hold different cases.  ('tie', i): every non-empty subset at tie_m[i]; ('thr', k, up): every subset at
    THR4[k] (up: just above it; the fourth threshold has no such copy); 'hot'; then three copies of the short block:
    'row_end' has its cases 5 and 6 in one pair on two rows (N is odd: cell (r + 1) N - 1 of an even row r is even),
    'wave_end' has case 4 in the last cell of a 128-cell wave of the pair kernels and case 5 in the first cell of the
    next, 'tail' ends in the tail cell N N - 1"""
    n, at, c = N * N, {}, 1
    names = ([(('tie', i), 2 ** P - 1) for i in range(4)] + [(('thr', k, up), 2 ** P) for k, up in THR_BLOCKS]
             + [('hot', HOT_SPAN)])
    for name, length in names:
        c |= 1
        at[name] = c
        c += length
    r = 0
    while (r + 1) * N - 6 < c:
        r += 2
    at['row_end'] = (r + 1) * N - 6
    c = at['row_end'] + SHORT
    at['wave_end'] = c + (123 - c) % 128
    at['tail'] = n - SHORT
    assert at['wave_end'] + SHORT <= at['tail'] - 128 and all(v % 2 == 1 for v in at.values())
    return at


def hot_cells(N, P):
    """even and odd cells, pairs with one hot cell and with two"""
    return layout(N, P)['hot'] + 2 * np.arange(HOT) + np.arange(HOT) // 7


@lru_cache(maxsize=None)
def plan_members(N, P):
    """six members of P plans, weights WEIGHTS: the blocks of layout(N, P), the plans rotated from member to member
    (so the regret at a cell moves through 0, one ulp, m / 2 and m), the first two the same, the last one zero in
    every plan.  At the HOT cells plan 0 holds 2^21 and plan 1 that less 1e6 (1 + k c 2^-40), k = 0, 0, 1, 2, 3 over
    the members: the regret of plan 1 is a large mean with a tiny spread until the last member's zero.  In member 3
    the tail cell is the only cell of the last wave that holds anything
    -> list of (name, fields [P, N, N], profile, weight, negval)"""
    n, at = N * N, layout(N, P)
    hot = hot_cells(N, P)
    out = []
    for (name, rot, profile, negval, whole_tail), w in zip(_SEQ, WEIGHTS):
        F = np.zeros((P, n))
        if rot is not None:
            for i, m in enumerate(tie_m(rot)):
                F[:, at['tie', i]:at['tie', i] + 2 ** P - 1] = tie_block(P, m, i)
            for k, up in THR_BLOCKS:
                F[:, at['thr', k, up]:at['thr', k, up] + 2 ** P] = thr_block(P, THR4[k], up)
            sb = short_block(P)
            for where in ('row_end', 'wave_end', 'tail'):
                F[:, at[where]:at[where] + SHORT] = sb
            if not whole_tail:
                F[:, at['tail']:n - 1] = 0.0
            F = F[(np.arange(P) + rot) % P]
            F[0, hot] = 2.0 ** 21
            F[1, hot] = 2.0 ** 21 - 1e6 * (1.0 + rot * (np.arange(HOT) + 1.0) * 2.0 ** -40)
        assert np.isfinite(F).all() and (F >= 0).all()
        out.append((name, F.reshape(P, N, N), profile, w, negval))
    assert np.array_equal(out[0][1], out[1][1]) and not out[-1][1].any()
    return out


def bump_plans(N, P):
    """what a model gives: one smooth bump scaled per plan, the last plan the largest; above zero no value meets
    another (the 'sum' profile has a slot of zeros, as most of a model's domain is: a P-fold tie at zero)"""
    b = CF.bump(N)
    scale = [0.5 + j / 16.0 + j / 1024.0 for j in range(P)]
    return [('bump', np.array([b * s for s in scale]), p, 1, NEGVAL) for p in ('rising', 'falling', 'sum')]


# ---- the contrast zoo -----------------------------------------------------------------------------------------------

def pair_cases():
    """[2, cases] of (a, b), an even number of them"""
    c = []
    for t in CF.THR:
        lo = math.nextafter(t, 0.0)
        c += [(t, lo), (lo, t), (t, t)]
    c += [(25.0, 25.0), (0.75, 0.75)]                               # d = 0: neither sign plane counts
    for m in (25.0, 1e300, SUBNORMAL):
        c += [(m, math.nextafter(m, 0.0)), (math.nextafter(m, 0.0), m)]       # one ulp, either sign
    c += [(1e16, 1.0), (1.0, 1e16)]                                 # a - b rounds
    c += [(150.0, 0.0), (0.0, 150.0), (1e-300, 3e-300)]
    assert len(c) % 2 == 0
    return np.array(c).T


PAIR_LOG = 1500            # the cells of the loguniform member
_PAIR_SEQ = (('base', 0, 'sum', 0.0), ('base again', 0, 'sum', 0.0), ('rot1', 1, 'cut', NEGVAL),
             ('rot2 log', 2, 'rising', 0.0), ('rot3', 3, 'prob', 0.0), ('zero', None, 'falling', NEGVAL))


@lru_cache(maxsize=None)
def pair_layout(N):
    """the first cells of the four copies of the case block: in the open, across a row end (cases 5 and 6 in one pair
    on two rows), across the end of a 128-cell wave (case 4 its last cell), and ending in the tail cell"""
    n, L = N * N, pair_cases().shape[1]
    at = {'open': PAIR_LOG + 1}
    c = at['open'] + L
    r = 0
    while (r + 1) * N - 6 < c:
        r += 2
    at['row_end'] = (r + 1) * N - 6
    c = at['row_end'] + L
    at['wave_end'] = c + (123 - c) % 128
    at['tail'] = n - L
    assert at['wave_end'] + L <= at['tail'] - 128 and all(v % 2 == 1 for v in at.values())
    return at


@lru_cache(maxsize=None)
def pair_members(N):
    """six members (a, b), weights WEIGHTS: the case block at its four places, the cases moved on by one cell from
    member to member -- so d changes sign at a cell and the mean crosses zero --, the first two members the same -- so
    a negative d repeats under a negative mean and nothing is stored --, in member 3 also 1500 cells of the loguniform
    field against a fixed permutation of themselves and only the last case of the tail block, the last member zero
    -> list of (name, fields [2, N, N], profile, weight, negval)"""
    n, at, cases = N * N, pair_layout(N), pair_cases()
    L = cases.shape[1]
    lu = CF.zoo(N)['loguniform'].ravel()[:PAIR_LOG]
    perm = np.random.default_rng(CF.SEED).permutation(PAIR_LOG)
    out = []
    for (name, rot, profile, negval), w in zip(_PAIR_SEQ, WEIGHTS):
        F = np.zeros((2, n))
        if rot is not None:
            blk = np.roll(cases, rot, axis=1)
            for where in at:
                F[:, at[where]:at[where] + L] = blk
            if rot == 2:
                F[0, :PAIR_LOG], F[1, :PAIR_LOG] = lu, lu[perm]
                F[:, at['tail']:n - 1] = 0.0
        out.append((name, F.reshape(2, N, N), profile, w, negval))
    assert np.array_equal(out[0][1], out[1][1]) and not out[-1][1].any()
    return out


def bump_pairs(N):
    b = CF.bump(N)
    return [('bump', np.array([b, b * 0.875]), p, 1, NEGVAL) for p in ('rising', 'falling', 'sum')]


# ---- the rules of the header, restated ------------------------------------------------------------------------------

def values(member, e):
    """[P, n]: what the plans of a member hold in entry e of its profile"""
    _name, F, profile, _w, negval = member
    stat, post = CF.PROFILES[profile]
    return np.array([CF.record_value(f, stat[e], post[e], negval).ravel() for f in F])


def _pairs_alike(a):
    a = a.copy()
    k = a.shape[1] // 2 * 2
    a[:, 1:k:2] = a[:, 0:k:2]
    return a


def rank_planes(a, thr, alter=None):
    """one member in one slot, a [P, n]: m = max_j a_j, n_max the plans at m; best_j: a_j == m and n_max == 1;
    regret r_j = m - a_j; per threshold, with c the plans at a_j >= t: sole_j: a_j >= t and c == 1, any: c >= 1,
    all: c == P; rows[j][k]: the cells with a_j >= t_k.  alter: one of RANK_RULES, the altered rule"""
    a = np.asarray(a, dtype=np.float64)
    if alter == 'pair':
        a = _pairs_alike(a)
    P = a.shape[0]
    m = (a[:-1] if alter == 'no_last' else a).max(0)
    hold = a == m
    if alter == 'tie_lowest':
        best = hold & (np.cumsum(hold, 0) == 1)
    elif alter == 'tie_all':
        best = hold
    else:
        best = hold & (hold.sum(0) == 1)
    reg = np.array([np.delete(a, j, 0).max(0) - a[j] for j in range(P)]) if alter == 'others' else m - a
    t = np.asarray(thr, dtype=np.float64).reshape(-1, 1, 1)
    ge = (a[None] > t) if alter == 'gt' else (a[None] >= t)
    c = ge.sum(1)
    sole = ge & ((c >= 1) if alter == 'sole_any' else (c == 1))[:, None]
    rows = ge.sum(2).T
    if alter == 'tail_twice':
        rows = rows + ge[:, :, -1].T
    return {'reg': reg, 'best': best, 'sole': sole, 'any': c >= 1, 'all': (c >= P - 1) if alter == 'all_but_one' else (c == P),
            'rows': rows}


def contrast_planes(ab, thr, alter=None):
    """one member in one slot, ab [2, n]: d = a - b; pos: d > 0; neg: d < 0; gain_k: a >= t_k and b < t_k; loss_k:
    b >= t_k and a < t_k; rows[side][k]: the cells with a >= t_k, then with b >= t_k"""
    ab = np.asarray(ab, dtype=np.float64)
    if alter == 'pair':
        ab = _pairs_alike(ab)
    a, b = ab
    d = a - b
    t = np.asarray(thr, dtype=np.float64).reshape(-1, 1)
    ga, gb = ((a > t), (b > t)) if alter == 'gt' else ((a >= t), (b >= t))
    gain = ga & ((b <= t) if alter == 'gain_le' else ~gb)
    rows = np.array([ga.sum(1), gb.sum(1)])
    if alter == 'tail_twice':
        rows = rows + np.array([ga[:, -1], gb[:, -1]])
    return {'d': d, 'pos': (d >= 0) if alter == 'ge0' else (d > 0), 'neg': d < 0, 'gain': gain, 'loss': gb & ~ga, 'rows': rows}


def rank_count_planes(cnt, P, nthr):
    """the count planes in the device's order: best_0 .. best_{P-1}, then per k sole_k0 .. sole_k,P-1, any_k, all_k"""
    out = [cnt['best'][j] for j in range(P)]
    for k in range(nthr):
        out += [cnt['sole'][k, j] for j in range(P)] + [cnt['any'][k], cnt['all'][k]]
    return out


def contrast_count_planes(cnt, nthr):
    """pos, neg, gain_0, loss_0, gain_1, ..."""
    out = [cnt['pos'], cnt['neg']]
    for k in range(nthr):
        out += [cnt['gain'][k], cnt['loss'][k]]
    return out


def assemble(entries, S, chunk=None):
    """the planes of a handle of S slots from those of the five entries; chunk: the altered launch that writes the
    slots of a later chunk to slot - chunk"""
    out = [np.zeros_like(entries[0]) for _ in range(S)]
    for s in range(S):
        out[s - chunk if chunk and s >= chunk else s] += entries[entry_of(s)]
    return out


RANK_RULES = {'tie_lowest': 'a tie goes to the lowest index', 'tie_all': 'a tie goes to every holder',
              'gt': '> for >= at a threshold', 'sole_any': 'sole with n >= 1', 'all_but_one': 'all with n >= P - 1',
              'others': 'regret against the maximum of the other plans', 'tail_twice': "the rows count the tail item's missing second cell",
              'chunk': 'the slots of a second chunk written to slot - chunk', 'pair': "the second cell of a pair takes the first cell's values",
              'no_last': 'the last plan left out of the maximum'}
CONTRAST_RULES = {'gt': '> for >= at a threshold', 'ge0': 'd >= 0 for d > 0', 'gain_le': 'gain with b <= t',
                  'tail_twice': "the rows count the tail item's missing second cell", 'pair': "the second cell of a pair takes the first cell's values"}


# ---- the moments ----------------------------------------------------------------------------------------------------

_MOMENTS = {}


def moments(V, weights=WEIGHTS, half=HALF):
    """V [M, n], the regrets or differences of the members at every cell -> dict of (mean [n], M2 [n]): 'plain' and
    'fused' (crafted_fields.welford), 'first2' after two members, 'ab' / 'ba' the members 0 .. half - 1 and the rest
    accumulated alone and merged as first += last and last += first (merge_fused); and 'at' [u], one cell of every
    distinct column, with 'exact' = exact_moments of those columns.  Computed once per distinct column"""
    V = np.ascontiguousarray(V, dtype=np.float64)
    Vu, at, inv = np.unique(V, axis=1, return_index=True, return_inverse=True)
    inv = np.asarray(inv).ravel()
    key = (Vu.tobytes(), Vu.shape, tuple(weights), half)
    if key not in _MOMENTS:
        w = list(weights)
        with np.errstate(over='ignore', invalid='ignore'):
            head, tail = CF.welford(Vu[:half], w[:half], True), CF.welford(Vu[half:], w[half:], True)
            Wh, Wt = sum(w[:half]), sum(w[half:])
            _MOMENTS[key] = {'plain': CF.welford(Vu, w, False), 'fused': CF.welford(Vu, w, True),
                             'first2': CF.welford(Vu[:2], w[:2], True), 'ab': CF.merge_fused(head, tail, Wh, Wt),
                             'ba': CF.merge_fused(tail, head, Wt, Wh), 'exact': CF.exact_moments(Vu, w)}
    u = _MOMENTS[key]
    out = {k: (u[k][0][inv], u[k][1][inv]) for k in ('plain', 'fused', 'first2', 'ab', 'ba')}
    out['at'], out['exact'] = at, u['exact']
    return out


def moment_errors(mean, M2, exact):
    """as crafted_fields.moment_errors, with both units floored at 2^-1075 and an infinite M2 admitted where
    sum w v^2 is beyond the largest double (and then not measured); M2 may hold floats or Fractions"""
    em, eq, um, uq = exact
    worst_m = worst_q = Fraction(0)
    for i in range(len(um)):
        if um[i] == 0:
            assert mean[i] == 0 and M2[i] == 0, i
            continue
        worst_m = max(worst_m, abs(Fraction(mean[i]) - em[i]) / max(um[i], FLOOR))
        if isinstance(M2[i], float) and math.isinf(M2[i]):
            assert M2[i] > 0 and uq[i] * 2 ** 53 >= 2 ** 1023, i
            continue
        worst_q = max(worst_q, abs(Fraction(M2[i]) - eq[i]) / max(uq[i], FLOOR))
    return float(worst_m), float(worst_q)


def _accumulate(mem, planes, keys):
    """per entry: the weighted sums of the boolean planes `keys`, the rows [member, ...] and the per-member values"""
    out = []
    for e in range(NENTRY):
        per = [planes(values(m, e)) for m in mem]
        ent = {k: sum(int(m[3]) * p[k].astype(np.int64) for m, p in zip(mem, per)) for k in keys}
        ent['rows'] = np.array([p['rows'] for p in per], dtype=np.int64)
        ent['per'] = per
        out.append(ent)
    return out


@lru_cache(maxsize=None)
def rank_reference(N, P):
    """per entry e: best [P, n], sole [4, P, n], any / all [4, n] weighted counts for the thresholds THR4, rows
    [member, P, 4], and 'mom' [P]: moments() of the regrets of every plan"""
    mem = plan_members(N, P)
    ref = _accumulate(mem, lambda a: rank_planes(a, THR4), ('best', 'sole', 'any', 'all'))
    for ent in ref:
        ent['mom'] = [moments(np.array([p['reg'][j] for p in ent['per']])) for j in range(P)]
        del ent['per']
    return ref


@lru_cache(maxsize=None)
def contrast_reference(N):
    """per entry e: pos / neg [n], gain / loss [4, n] weighted counts, rows [member, 2, 4], and 'mom': moments()
    of d"""
    mem = pair_members(N)
    ref = _accumulate(mem, lambda ab: contrast_planes(ab, THR4), ('pos', 'neg', 'gain', 'loss'))
    for ent in ref:
        ent['mom'] = moments(np.array([p['d'] for p in ent['per']]))
        del ent['per']
    return ref


# ---- the release plans: the ring ------------------------------------------------------------------------------------

def ring(N):
    """the whole outer border with a value of its own in every cell -- the four corners, the cell before and after
    every row end --, and the second cell of every row, so that a flat-index wrap of any shift shows in every row"""
    f = np.zeros((N, N))
    edge = np.zeros((N, N), dtype=bool)
    edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = edge[:, 1] = True
    f[edge] = 1.0 + np.arange(int(edge.sum())) / 7.0
    return f


def ring_plans(N):
    """single-group plans: list of [(drow, dcol, amount), ...]"""
    M = N - 1
    one = [(0, 0), (0, 1), (0, -1), (1, 0), (-1, 0), (0, M), (0, -M), (M, 0), (-M, 0), (M, -M)]
    return [[(r, c, 1.0)] for r, c in one] + [[(0, 0, 1.0), (1, -2, 0.75), (-3, M, 1.0 / 3.0)]]


def shifted(v, dr, dc):
    """out(r, c) = v(r - dr, c - dc), 0 where the source row or column lies outside the domain"""
    N = v.shape[0]
    out = np.zeros_like(v)
    r0, r1, c0, c1 = max(dr, 0), min(N, N + dr), max(dc, 0), min(N, N + dc)
    out[r0:r1, c0:c1] = v[r0 - dr:r1 - dr, c0 - dc:c1 - dc]
    return out


def sites_expected(v, plan):
    """Y = Y + amount * shifted(v) from +0.0, the sites in order, product and sum rounded separately"""
    Y = np.zeros_like(v)
    for dr, dc, amount in plan:
        Y = Y + np.float64(amount) * shifted(v, dr, dc)
    return Y
