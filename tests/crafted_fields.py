"""Crafted fields for the value-level accumulators (ps_summary, ps_hist, ps_arrival, ps_peak, ps_excur, ps_range),
the slot descriptors that turn one field into a history over NSLOT slots, and references that share nothing with the
library: plain numpy restatements of the header's rules (every + - x / of an IEEE double is the same in numpy and on
the device), Python integers and fractions.Fraction where one rounding of an exact result is needed.  Shared by
test_crafted_fields_cpu.py and test_crafted_fields_gpu.py; written so that other handles can be fed the same members.

A *field* is an [N, N] float64 array of zeros and positive finite values.  A *profile* is a pair (stat_scale, post_scale)
of NSLOT numbers: slot s holds record_value(field, stat[s], post[s]), the rule of ps_summary_add with delta = 0.  A
*member* is (name, field, profile name, weight 1..3).  N = 65 (N * N = 66 * 64 + 1) and 129 (260 * 64 + 1): the tail
cell has no partner, the last wave and the last mask word hold one real cell, every kernel has more than one block.

Fractions.  The header admits range fractions in (0, 1) only, so the place of p = 1 is taken by the largest double
below 1: for Q < 2^53 -- every field here -- the smallest integer >= p Q is then Q itself, the whole mass.

plateau2 / plateau2_odd.  One field cannot put the need of one listed fraction on a plateau boundary and that of
another one unit beyond the same boundary: two needs differ by (p_b - p_a) Q, and Q >= 2^36.  plateau2 has the need
of 0.5 exactly on the boundary (200 cells at 1.0 below 100 cells at 2.0); plateau2_odd has three cells, 1 + 2^-36 and
twice 0.5 + 2^-36, Q = 2^37 + 3, so that the need of 0.5 is the mass of the top cell plus one unit.

Summary restatement against the exact rational moments, the largest over summary_members() at both sizes (measured
by test_crafted_fields_cpu.py, which asserts them with a margin of 2; the inputs are fixed and only + - x / are used):
    mean, in units of 2^-53 * max_m |v_m|:    1.0492 (MEAN_ERR), the plain and the fused restatement alike
    M2, in units of 2^-53 * sum_m w_m v_m^2:  2.3235 plain, 2.4446 (M2_ERR) with the last step fused
"""
import math
from fractions import Fraction
from functools import lru_cache

import numpy as np

from parasitoids_amd.predictive import NEGVAL

MEAN_ERR = 1.0492
M2_ERR = 2.4446

SIZES = (65, 129)
NSLOT = 5
THR = (1.0, 10.0, 100.0)
EDGES = (1e-3, 1e-2, 1e-1, 1.0, 10.0, 100.0, 1e3)
FRACTIONS = (2.0 ** -10, 0.5, 0.95, math.nextafter(1.0, 0.0))
SUM_WEIGHTS = (1, 3, 2, 1, 2)
SEED = 20261021

_Z, _O = (0.0,) * NSLOT, (1.0,) * NSLOT
PROFILES = {
    'rising': (_O, (1 / 16, 1 / 8, 1 / 4, 1 / 2, 1.0)),
    'falling': (_O, (1.0, 1 / 2, 1 / 4, 1 / 8, 1 / 16)),
    'tie': (_O, (1 / 4, 1.0, 1 / 2, 1.0, 1 / 4)),                   # (1, 4, 2, 4, 1) / 4: the peak ties in time
    'recross': ((1.0, 1.0, 1.0, 0.0, 0.0), (1.0, 1 / 4, 1.0, 1.0, 1.0)),   # (4, 1, 4) / 4: drops below and comes back
    'flat': ((1.0, 1.0, 1.0, 0.0, 0.0), (2.0, 2.0, 2.0, 1.0, 1.0)),        # (2, 2, 2)
    'late': ((0.0, 0.0, 1.0, 0.0, 0.0), _O),                               # (0, 0, 1, 0)
    # through the cut the history depends on the cell: r * 2^-30 >= negval peaks at slot 0 with 2 r, the rest at slot 1
    'cut': ((2.0 ** -30, 1.0, 0.0, 0.0, 0.0), (2.0 ** 31, 1.0, 1.0, 1.0, 1.0)),
    'prob': ((1.0, 2.0, 4.0, 2.0, 1.0), (1 / 130000,) * NSLOT),            # a post-scale that is no power of two
    # the summary group: exact scalings, the cut, the prob_model scale, a slot of zeros
    'sum': ((1.0, 2.0 ** -30, 1.0, 0.0, 1.0), (1.0, 2.0 ** 31, 1 / 130000, 1.0, 1 / 4)),
}
RANGE_PROFILE = ((1.0, 2.0 ** -30), (1.0, 2.0 ** 31))      # ps_range: the field itself, and what the cut leaves of it


def around(x):
    return (math.nextafter(x, 0.0), float(x), math.nextafter(x, math.inf))


def record_value(r, stat_scale, post_scale, negval=NEGVAL, strict=False):
    """t = r * stat_scale;  v = (t != 0 and not (t < negval)) ? (t + 0) * post_scale : 0   (delta = 0).  strict: the
    altered rule t > negval"""
    t = np.asarray(r, dtype=np.float64) * np.float64(stat_scale)
    keep = (t > negval) if strict else ((t != 0.0) & ~(t < negval))
    return np.where(keep, (t + 0.0) * np.float64(post_scale), 0.0)


def record_value_exact(r, stat_scale, post_scale, negval=NEGVAL):
    """the same for one Python float, every product rounded once from the exact rational"""
    t = float(Fraction(r) * Fraction(stat_scale))
    if t == 0.0 or t < negval:
        return 0.0
    return float(Fraction(t) * Fraction(post_scale))


def history(field, profile, negval=NEGVAL, strict=False):
    """[nslot, N, N]: the values of the slots of one member"""
    stat, post = PROFILES[profile] if isinstance(profile, str) else profile
    return np.array([record_value(field, a, b, negval, strict) for a, b in zip(stat, post)])


# ---- the zoo --------------------------------------------------------------------------------------------------------

def spots(N, i):
    """the cells that hold value i of a family: an even cell, an odd cell, both cells of a pair, a pair that straddles
    a row end (N is odd: cell (r + 1) N - 1 of an even row r is even), the last two cells of a 64-cell wave and the
    first of the next (for odd i also of a 128-cell wave of the pair kernels)"""
    b = 64 * (i + 1)
    e = (22 + 2 * i + 1) * N - 1
    assert e % 2 == 0 and e + 1 < N * N - 1 and b + 64 < 22 * N
    return {'even': [b + 2], 'odd': [b + 7], 'pair': [b + 10, b + 11], 'row_end': [e, e + 1],
            'wave_end': [b + 62, b + 63, b + 64]}


def family(N, values):
    """one field per value: every value at its spots in each of them, and value i in the tail cell of field i"""
    base = np.zeros(N * N)
    for i, v in enumerate(values):
        for cells in spots(N, i).values():
            base[cells] = v
    out = []
    for v in values:
        f = base.copy()
        f[-1] = v
        out.append(f.reshape(N, N))
    return out


PAIR_VALUES = tuple(0.5 * e for e in EDGES) + (2.0 * EDGES[-1],)       # one value inside each of the bins 0 .. B + 1
PAIR_BASE = 512                                                          # cells 512 .. 639: one wave of a pair kernel


def _ramp(N, top, scale=1.0):
    """256 cells with top * k / 257, k = 1 .. 256, spread over the whole domain, and the maximum `top` at cell 4100 (in
    the second 4096-cell block); everything times scale"""
    f = np.zeros(N * N)
    cells = (np.arange(256) * ((N * N - 1) // 256)) + 1
    f[cells] = np.arange(1, 257) / 257.0 * 32.0
    f[4100] = top
    return (f * scale).reshape(N, N)


@lru_cache(maxsize=None)
def zoo(N):
    """-> dict name -> [N, N] field, in a fixed order"""
    n = N * N
    Z = {}

    def flat(name, cells, values):
        f = np.zeros(n)
        f[cells] = values
        Z[name] = f.reshape(N, N)
    flat('zero', [], 0.0)
    flat('first_cell', [0], 25.0)
    flat('tail_cell', [n - 1], 25.0)
    Z['full'] = np.full((N, N), 150.0)      # at or above the top threshold in some slots of most profiles: whole waves
                                            # arrive before the last slot
    for i, f in enumerate(family(N, [x for t in THR for x in around(t)])):
        Z['at_thresholds/%d' % i] = f
    for i, f in enumerate(family(N, [x for e in EDGES for x in around(e)])):
        Z['at_edges/%d' % i] = f
    # around negval itself, and around negval * 2^30, which the 'cut' and 'sum' profiles' 2^-30 carries across it
    for i, f in enumerate(family(N, list(around(NEGVAL)) + [x * 2.0 ** 30 for x in around(NEGVAL)])):
        Z['at_negval/%d' % i] = f
    a, b = np.zeros(64), np.zeros(64)
    for p in range(64):
        a[p] = PAIR_VALUES[p % 8]
        b[p] = PAIR_VALUES[(p + 1 + (p // 8) % 7) % 8]
        if p % 4 == 3:
            b[p] = 0.0
        if p % 8 == 5:
            a[p] = 0.0
    flat('split_pairs', np.arange(PAIR_BASE, PAIR_BASE + 128), np.stack([a, b], 1).ravel())
    e = np.array([PAIR_VALUES[p % 8] if p % 16 else 0.0 for p in range(64)])
    flat('equal_pairs', np.arange(PAIR_BASE, PAIR_BASE + 128), np.repeat(e, 2))
    rng = np.random.default_rng(SEED + N)
    f = 10.0 ** rng.uniform(-20.0, 20.0, n)
    f[rng.random(n) < 0.3] = 0.0
    Z['loguniform'] = f.reshape(N, N)
    # the range fields
    cells = np.arange(300) * (n // 300)
    flat('plateau2', cells, np.where(np.arange(300) % 3 == 0, 2.0, 1.0))
    flat('plateau2_odd', [0, 4097, n - 1], [0.5 + 2.0 ** -36, 1.0 + 2.0 ** -36, 0.5 + 2.0 ** -36])
    Z['all_equal'] = np.full((N, N), 0.75)
    # maximum 1.5 * 2^16, so that 2^(E - 36) = 2^-20 and the cells far below it, 2^-24, still pass the cut at negval
    lo = around(2.0 ** -20)
    flat('span36', [4099] + list(range(10, 90)) + [n - 1 - k for k in range(80)],
         [1.5 * 2.0 ** 16] + [(lo + (2.0 ** -24,))[k % 4] for k in range(160)])
    Z['pow2_max'] = _ramp(N, 32.0)
    Z['below_pow2_max'] = _ramp(N, math.nextafter(32.0, 0.0))
    Z['tiny'] = _ramp(N, 32.0, 1e-300 / 32.0)
    f = np.zeros(n)
    f[(np.arange(256) * ((n - 1) // 256)) + 1] = (10120 * np.arange(1, 257) // 257) * 5e-324
    f[4100] = 5e-320
    Z['subnormal_max'] = f.reshape(N, N)
    Z['big'] = _ramp(N, 32.0, 1e300 / 32.0)
    for name, f in Z.items():
        assert f.shape == (N, N) and np.isfinite(f).all() and (f >= 0).all(), name
    return Z


RANGE_FIELDS = ('zero', 'first_cell', 'tail_cell', 'full', 'plateau2', 'plateau2_odd', 'all_equal', 'span36', 'pow2_max',
                'below_pow2_max', 'tiny', 'subnormal_max', 'big', 'loguniform', 'at_negval/4')
EVERY_PROFILE = ('at_thresholds/4', 'at_negval/1', 'at_negval/4', 'split_pairs', 'equal_pairs', 'loguniform')
SLOT_PROFILES = ('rising', 'falling', 'tie', 'recross', 'flat', 'late', 'cut', 'prob')


@lru_cache(maxsize=None)
def members(N):
    """the members of the slot handles: every field once with a profile by rotation (the first two, 'zero' under
    'rising', twice: two identical members, and an empty one), the fields of EVERY_PROFILE under every profile, 'full'
    under three more ->
    list of (name, field, profile, weight 1..3)"""
    Z = zoo(N)
    out = [('zero', Z['zero'], 'rising')]
    for i, (name, f) in enumerate(Z.items()):
        out.append((name, f, SLOT_PROFILES[i % len(SLOT_PROFILES)]))
    for name in EVERY_PROFILE:
        out.extend((name, Z[name], p) for p in SLOT_PROFILES)
    out.extend(('full', Z['full'], p) for p in ('tie', 'recross', 'flat'))
    return [(n, f, p, 1 + i % 3) for i, (n, f, p) in enumerate(out)]


@lru_cache(maxsize=None)
def histories(N):
    """[member][NSLOT, N, N]"""
    return [history(f, p) for _n, f, p, _w in members(N)]


def range_members(N):
    """-> list of (name, field, RANGE_PROFILE, weight, negval): negval = 0 for the two fields that lie wholly below the
    package's, which would cut them to nothing"""
    return [(name, zoo(N)[name], RANGE_PROFILE, 1 + i % 3, 0.0 if name in ('tiny', 'subnormal_max') else NEGVAL)
            for i, name in enumerate(RANGE_FIELDS)]


HOT = 200      # cells of the large-mean-tiny-spread group, the rows 40 and up of either size


def summary_members(N):
    """five members, weights SUM_WEIGHTS, all under the 'sum' profile.  The first two are the same field: after them
    mean == v and M2 == 0 bit for bit, and the second stores nothing.  HOT cells hold 1e6 (1 + k (j + 1) 2^-40) across
    the members, k = 0, 0, 1, 2, 3"""
    Z = zoo(N)
    base = [Z['at_thresholds/4'], None, Z['loguniform'], Z['split_pairs'] + Z['at_negval/4'],     # no cell in both
            np.where(Z['at_edges/10'] > 0, Z['at_edges/10'], Z['full'])]
    base[1] = base[0]
    out = []
    hot = 40 * N + 2 * np.arange(HOT) + np.arange(HOT) // 7      # even and odd cells, pairs with one hot cell and two
    for k, f in zip((0, 0, 1, 2, 3), base):
        g = f.copy().ravel()
        g[hot] = 1e6 * (1.0 + k * (np.arange(HOT) + 1.0) * 2.0 ** -40)
        out.append(g.reshape(N, N))
    assert np.array_equal(out[0], out[1])
    return [('sum%d' % i, f, 'sum', w) for i, (f, w) in enumerate(zip(out, SUM_WEIGHTS))]


def bump(N):
    """a smooth Gaussian bump, the shape of a model field: positive, centred, values that coincide with nothing"""
    y, x = np.mgrid[0:N, 0:N]
    cx, cy = (N - 1) / 2.0 + 0.3183098861, (N - 1) / 2.0 + 0.7071067811       # no two cells at one distance
    return 537.1 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * (N / 8.0) ** 2))


# ---- the summary: restatement and exact moments ---------------------------------------------------------------------

def fma(a, b, c):
    """a * b + c with one rounding: the exact value as a ratio of integers (every denominator is a power of two), and
    Python's integer true division, which rounds correctly.  An infinite argument gives what IEEE arithmetic gives
    (no rounding is left to do), and a result beyond the largest double is the infinity of its sign"""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    (na, da), (nb, db), (nc, dc) = a.as_integer_ratio(), b.as_integer_ratio(), c.as_integer_ratio()
    num = na * nb * dc + nc * da * db
    try:
        return num / (da * db * dc)
    except OverflowError:
        return math.inf if num > 0 else -math.inf


def welford(values, weights, fused):
    """values [M, n]: the header's statement per cell, members in order --
        W' = W + w;  d = v - mean;  d == 0: nothing;  mean += d w / W';  M2 += w d (v - mean)
    d w / W' is (d * w) / W'.  fused: the last line as fma(w * d, v - mean, M2), one rounding of the exact result, what
    contraction within the expression makes of it.  -> (mean [n], M2 [n])"""
    V = np.asarray(values, dtype=np.float64)
    mean, M2 = np.zeros(V.shape[1]), np.zeros(V.shape[1])
    W = 0
    for v, w in zip(V, weights):
        W += int(w)
        d = v - mean
        new = mean + d * float(w) / float(W)
        new = np.where(d == 0.0, mean, new)
        a, b = float(w) * d, v - new
        if fused:
            upd = M2.copy()
            for i in np.flatnonzero(d != 0.0):
                upd[i] = fma(float(a[i]), float(b[i]), float(M2[i]))
        else:
            upd = np.where(d == 0.0, M2, M2 + a * b)
        mean, M2 = new, upd
    return mean, M2


def merge_fused(a, b, Wa, Wb):
    """dst = a (mean, M2, weight Wa) += src = b, as k_summary_merge computes Chan, Golub & LeVeque's update (read off
    the gfx950 code of `ma + d * (Wb / W)` and `qa + qb + d * d * (Wa * Wb / W)` under -ffp-contract=on):
        d = mean_b - mean_a;  mean = fma(d, Wb / W, mean_a);  M2 = fma(d * d, (Wa * Wb) / W, M2_a + M2_b)"""
    (ma, qa), (mb, qb) = a, b
    W = float(Wa) + float(Wb)
    d, c1, c2, q = mb - ma, float(Wb) / W, float(Wa) * float(Wb) / W, qa + qb
    mean, M2 = ma.copy(), q.copy()
    for i in np.flatnonzero(d != 0.0):
        mean[i] = fma(float(d[i]), c1, float(ma[i]))
        M2[i] = fma(float(d[i] * d[i]), c2, float(q[i]))
    return mean, M2


def exact_moments(values, weights):
    """-> (mean, M2, um, uq) [n] as Fractions in object arrays, all in integers: sum w v / W, sum w (v - mean)^2, and
    the two units 2^-53 max_m |v_m| and 2^-53 sum_m w_m v_m^2 (0 where the cell holds nothing)"""
    V = np.asarray(values, dtype=np.float64)
    W = int(sum(weights))
    out = [np.zeros(V.shape[1], dtype=object) for _ in range(4)]
    for a in out:
        a[:] = Fraction(0)
    for i in np.flatnonzero(V.any(0)):
        r = [float(x).as_integer_ratio() for x in V[:, i]]
        D = max(den for _n, den in r)
        n = [num * (D // den) for num, den in r]
        S = sum(int(w) * x for w, x in zip(weights, n))
        S2 = sum(int(w) * x * x for w, x in zip(weights, n))
        out[0][i] = Fraction(S, W * D)
        out[1][i] = Fraction(W * S2 - S * S, W * D * D)
        out[2][i] = Fraction(max(abs(x) for x in n), D * 2 ** 53)
        out[3][i] = Fraction(S2, D * D * 2 ** 53)
    return tuple(out)


def moment_errors(mean, M2, exact):
    """the largest errors of (mean, M2) [n] (floats or Fractions) against exact = exact_moments(...): the mean in
    units of 2^-53 max_m |v_m|, M2 in units of 2^-53 sum_m w_m v_m^2; cells that hold nothing must be exactly 0"""
    em, eq, um, uq = exact
    live = um != 0
    assert not np.asarray(mean)[~live].any() and not np.asarray(M2)[~live].any()
    worst_m = worst_q = Fraction(0)
    for i in np.flatnonzero(live):
        worst_m = max(worst_m, abs(Fraction(mean[i]) - em[i]) / um[i])
        worst_q = max(worst_q, abs(Fraction(M2[i]) - eq[i]) / uq[i])
    return float(worst_m), float(worst_q)


@lru_cache(maxsize=None)
def summary_reference(N):
    """per slot: dict(V [5, n], plain (mean, M2), fused (mean, M2), pair (mean, M2) after the first two members, exact:
    exact_moments of the five, counts [K, n]: the weight of the members at or above each threshold, ab / ba: the first
    two members and the last three, each accumulated alone, merged as first += last and as last += first)"""
    mem = summary_members(N)
    H = [history(f, p).reshape(NSLOT, -1) for _n, f, p, _w in mem]
    out = []
    for s in range(NSLOT):
        V = np.array([h[s] for h in H])
        head, tail = welford(V[:2], SUM_WEIGHTS[:2], True), welford(V[2:], SUM_WEIGHTS[2:], True)
        Wh, Wt = sum(SUM_WEIGHTS[:2]), sum(SUM_WEIGHTS[2:])
        out.append({'V': V, 'ab': merge_fused(head, tail, Wh, Wt), 'ba': merge_fused(tail, head, Wt, Wh), 'plain': welford(V, SUM_WEIGHTS, False), 'fused': welford(V, SUM_WEIGHTS, True),
                    'pair': welford(V[:2], SUM_WEIGHTS[:2], True), 'exact': exact_moments(V, SUM_WEIGHTS),
                    'counts': np.array([sum(int(w) * (v >= t) for v, w in zip(V, SUM_WEIGHTS)) for t in THR])})
    return out


# ---- the range levels, once more, on a plain sort -------------------------------------------------------------------

def levels(field, fractions=FRACTIONS, floor=False, partial=False, min_mass=0):
    """-> (lam [J], n [J], Q, E) of one field by sorting Python numbers.  The three switches are the altered rules:
    floor: the needed mass rounded down; partial: a plateau enters cell by cell; min_mass = 1: every value > 0 has
    mass, not only those >= 2^(E - 36)"""
    vals = sorted((float(x) for x in np.asarray(field).ravel() if x > 0), reverse=True)
    if not vals:
        return [math.inf] * len(fractions), [0] * len(fractions), 0, 0
    E = math.frexp(vals[0])[1] - 1
    q = [max(int(Fraction(x) * Fraction(2) ** (36 - E)), min_mass) for x in vals]
    Q = sum(q)
    lam, n = [], []
    for p in fractions:
        x = Fraction(float(p)) * Q
        need = x.numerator // x.denominator if floor else -((-x.numerator) // x.denominator)
        run, at = 0, len(vals) - 1
        for i, m in enumerate(q):
            run += m
            if run >= max(need, 1):
                at = i
                break
        lam.append(vals[at])
        n.append(at + 1 if partial else sum(1 for y in vals if y >= vals[at]))
    return lam, n, Q, E


# ---- the device side ------------------------------------------------------------------------------------------------

class Injector:
    """one exact-mode solver of domain N whose state record takes the crafted fields (HipSolve.set_state, PS_REC_STATE)"""

    def __init__(self, N):
        from parasitoids_amd import _lib as L
        from parasitoids_amd import hip_lib
        from scipy import sparse
        self.L, self.lib, self.dev, self._coo = L, L.load(), L.default_device(), sparse.coo_matrix
        seed = np.zeros((N, N))
        seed[N // 2, N // 2] = 1.0
        self.s = hip_lib.HipSolve(sparse.coo_matrix(seed), [5, 5], mode='exact')
        self._keep = {}

    def inject(self, field):
        """the field as the solver's state; the device must hold it bit for bit"""
        self.s.set_state(self._coo(field))
        back = self.s.dense(self.L.REC_STATE, 0)
        assert np.array_equal(back, field) and np.array_equal(np.signbit(back), np.signbit(field))

    def slots(self, profile, negval=NEGVAL):
        """the descriptor arguments of every ps_*_add between the solver and the weight: every slot reads the state"""
        stat, post = PROFILES[profile] if isinstance(profile, str) else profile
        key = (tuple(stat), tuple(post), negval)
        if key not in self._keep:
            L, n = self.L, len(stat)
            arrs = (L.i32([L.REC_STATE] * n), L.i32([0] * n), L.f64(list(stat)), L.f64(list(post)), L.i32([0] * n))
            self._keep[key] = (arrs, (n, L.p_i32(arrs[0]), L.p_i32(arrs[1]), L.p_f64(arrs[2]), L.p_f64(arrs[3]),
                                      L.p_i32(arrs[4]), float(negval)))
        return self._keep[key][1]

    def close(self):
        self.s.close()
