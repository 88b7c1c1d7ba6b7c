"""The crafted fields of crafted_fields.py, without a GPU: the zoo holds every case it is there for (counted from the
references alone), it tells every altered rule from the true one where a smooth bump -- the shape of a model field --
tells few, and the references agree with plain loops and exact rational arithmetic.

Altered rules a smooth bump of the same size cannot tell from the true ones (printed by
test_the_zoo_discriminates_where_a_smooth_bump_does_not; this list is the gap the crafted fields close): at N = 65 and
129 alike, `>` for `>=`, side='left', the last slot of a tie, the floor in the needed mass, a plateau entering partly,
mass for every v > 0, the tail cell dropped, t > negval -- eight of ten.  It tells only the arrival rule "after which it
stays" (under a falling history) and the swapped pair.

Summary restatement against the exact rational moments, the largest over the summary group at both sizes:
    mean  1.0492 x 2^-53 max_m |v_m|        (plain and fused alike)
    M2    2.3235 x 2^-53 sum_m w_m v_m^2    plain,   2.4446 fused
"""
import bisect
import math

import numpy as np
import pytest

import arrival_ref as AR
import crafted_fields as CF
import excur_ref as XR
import hist_ref as HR
import peak_ref as PK
import range_ref as RR

MEAN_MEASURED = 1.0492
M2_MEASURED = 2.4446
EDGES = np.array(CF.EDGES)
B = len(CF.EDGES) - 1


def test_constants_are_the_packages():
    from parasitoids_amd import predictive
    assert CF.NEGVAL == predictive.NEGVAL == 1e-8
    assert CF.FRACTIONS[-1] < 1.0 and all(0 < p < 1 for p in CF.FRACTIONS)
    assert len(CF.EDGES) == 7 and CF.EDGES[0] == 1e-3 and CF.EDGES[-1] == 1e3
    for N in CF.SIZES:
        assert N * N % 64 == 1 and N * N > 4096 + 64


def test_record_value_is_one_rounding_per_product():
    """the numpy restatement against the rational one on every distinct (value, slot) of the zoo at N = 65"""
    Z = CF.zoo(65)
    vals = np.unique(np.concatenate([f.ravel() for name, f in Z.items() if name != 'loguniform']
                                    + [Z['loguniform'].ravel()[:300]]))
    seen = 0
    for stat, post in CF.PROFILES.values():
        for a, b in set(zip(stat, post)):
            got = CF.record_value(vals, a, b)
            for r, g in zip(vals.tolist(), got.tolist()):
                assert g == CF.record_value_exact(r, a, b), (r, a, b)
                seen += 1
    assert seen > 5000


# ---- the zoo is what it claims --------------------------------------------------------------------------------------

def _member(N, name, profile):
    for (n, _f, p, _w), h in zip(CF.members(N), CF.histories(N)):
        if n == name and p == profile:
            return h.reshape(CF.NSLOT, -1)
    raise KeyError((name, profile))


def _pairs(x):
    """[.., n] -> [.., n // 2, 2]: the cells a thread of a pair kernel owns (the tail cell left out)"""
    n = x.shape[-1] // 2 * 2
    return x[..., :n].reshape(x.shape[:-1] + (n // 2, 2))


@pytest.mark.parametrize('N', CF.SIZES)
def test_the_zoo_is_what_it_claims(N):
    Z, n = CF.zoo(N), N * N
    mem, H = CF.members(N), [h.reshape(CF.NSLOT, -1) for h in CF.histories(N)]
    assert Z['zero'].sum() == 0 and np.count_nonzero(Z['first_cell']) == 1 and Z['first_cell'].flat[0] > 0
    assert np.count_nonzero(Z['tail_cell']) == 1 and Z['tail_cell'].flat[n - 1] > 0
    assert len(np.unique(Z['full'])) == 1 and len(np.unique(Z['all_equal'])) == 1
    # values at, just below and just above every threshold, edge and negval: at an even cell, an odd one, both cells of
    # a pair, across a row end, across a wave end, and in the tail cell of one of the family's fields
    for fam, targets in (('at_thresholds', CF.THR), ('at_edges', CF.EDGES), ('at_negval', (CF.NEGVAL,))):
        values = [x for t in targets for x in CF.around(t)]
        for i, x in enumerate(values):
            f = Z['%s/%d' % (fam, i)].ravel()
            assert f[n - 1] == x
            sp = CF.spots(N, i)
            for cells in sp.values():
                assert (f[cells] == x).all()
            assert sp['even'][0] % 2 == 0 and sp['odd'][0] % 2 == 1 and sp['pair'][0] % 2 == 0
            e = sp['row_end'][0]
            assert e % 2 == 0 and e // N + 1 == (e + 1) // N                 # one pair, two rows
            assert sp['wave_end'][1] % 64 == 63 and sp['wave_end'][2] % 64 == 0
        assert any(CF.spots(N, i)['wave_end'][2] % 128 == 0 for i in range(len(values)))
    # the same through the slots: a slot with scale 1 keeps v == t, and the ties are exact
    h = _member(N, 'at_thresholds/4', 'tie')
    for t in CF.THR:
        for x in CF.around(t):
            assert (h[1] == x).sum() >= 9 and np.array_equal(h[1], h[3])
    # negval: t == negval stays, the value below it goes; r * 2^-30 crosses it in the 'cut' profile
    below, at, above = CF.around(CF.NEGVAL)
    f = Z['at_negval/1'].ravel()
    v = CF.record_value(f, 1.0, 1.0)
    assert ((f == at) & (v == at)).sum() >= 9 and ((f == below) & (v == 0)).sum() >= 8
    assert ((f == above) & (v == above)).sum() >= 8
    h = _member(N, 'at_negval/4', 'cut')
    big = Z['at_negval/4'].ravel()
    assert ((big == at * 2.0 ** 30) & (h[0] == 2 * big)).sum() >= 8
    assert ((big == below * 2.0 ** 30) & (h[0] == 0) & (h[1] == big)).sum() >= 8
    # the pair fields
    bs, be = np.searchsorted(EDGES, _pairs(Z['split_pairs'].ravel()), 'right'), \
        np.searchsorted(EDGES, _pairs(Z['equal_pairs'].ravel()), 'right')
    wave = slice(CF.PAIR_BASE // 2, CF.PAIR_BASE // 2 + 64)
    ps = _pairs(Z['split_pairs'].ravel())[wave]
    assert CF.PAIR_BASE % 128 == 0 and (be[wave, 0] == be[wave, 1]).all()
    assert ((bs[wave, 0] != bs[wave, 1]) | ((ps > 0).sum(1) == 1)).all() and (bs[wave, 0] != bs[wave, 1]).sum() >= 56
    assert ((ps > 0).sum(1) == 1).sum() >= 16 and set(bs[wave].ravel()) == set(range(B + 2)) == set(be[wave].ravel())
    for t in CF.THR:
        assert ((ps[:, 0] >= t) != (ps[:, 1] >= t)).any()
    h = _pairs(_member(N, 'split_pairs', 'cut'))[:, wave]
    a, p = AR.arrival_slots(h, CF.THR), PK.peak_slot(h)
    assert (p[:, 0] != p[:, 1]).sum() >= 8 and (a[..., 0] != a[..., 1]).any(1).all()
    # the histories: ties in time, re-crossings, slots of zeros, cells that reach only the lower thresholds, waves
    # that all pass the top threshold before the last slot (the arrival walk leaves early) and waves of which only a
    # part does
    ties = recross = lower_only = early = mixed = zero_slots = 0
    for (name, f, prof, w), h in zip(mem, H):
        m = h.max(0)
        ties += int(((h == m).sum(0) >= 2)[m > 0].sum())
        for t in CF.THR:
            hit = h >= t
            first = np.argmax(hit, 0)
            gone = np.array([(~hit[s]) & (s > first) & hit.any(0) for s in range(CF.NSLOT)])
            last = CF.NSLOT - 1 - np.argmax(hit[::-1], 0)
            recross += int((gone & (np.arange(CF.NSLOT)[:, None] < last)).any(0).sum())
        a = AR.arrival_slots(h, CF.THR)
        lower_only += int(((a[0] < CF.NSLOT) & (a[-1] == CF.NSLOT)).sum())
        top = np.zeros(((n + 127) // 128) * 128, dtype=np.int64) + CF.NSLOT
        top[:n] = a[-1]
        top[n:] = -1                                        # pad lanes are not live
        g = top.reshape(-1, 128)
        done = np.where(g < 0, 0, g).max(1)
        early += int((done < CF.NSLOT - 1).sum())
        mixed += int((((g >= 0) & (g < CF.NSLOT)).any(1) & (g == CF.NSLOT).any(1)).sum())
        zero_slots += int((~h.any(1)).sum())
    assert ties > 1000 and recross > 100 and lower_only > 1000 and early > 100 and mixed > 100 and zero_slots > 100
    # histogram: whole members in bin 0, values in bin B + 1, a pair in one bin and in two
    bins = [np.searchsorted(EDGES, h, 'right') for h in H]
    assert any((b == 0).all() for b in bins) and sum(int((b == B + 1).sum()) for b in bins) > 100
    assert sum(int((_pairs(b)[..., 0] != _pairs(b)[..., 1]).sum()) for b in bins) > 1000
    assert sum(int(((_pairs(b)[..., 0] == _pairs(b)[..., 1]) & (_pairs(b)[..., 0] > 0)).sum()) for b in bins) > 1000
    # excursion: an empty member, a full one, two identical ones
    assert not H[0].any() and np.array_equal(H[0], H[1]) and any((h >= CF.THR[0]).all(1).any() for h in H)
    # the range fields
    on_plateau = massless = 0
    for name, f, prof, w, negval in CF.range_members(N):
        for v in CF.history(f, prof, negval):
            lam, cnt, Q, E, _sets = RR.member_levels(v, CF.FRACTIONS)
            assert Q < 2 ** 53 and RR.needed_mass(CF.FRACTIONS[-1], Q) == Q
            if Q:
                on_plateau += sum(int((v == x).sum() > 1) for x in lam)
                massless += int(((v > 0) & (v < math.ldexp(1.0, E - 36))).sum())
    assert on_plateau >= 10 and massless >= 80
    q, Q, E = RR.integer_mass(Z['plateau2'])
    assert RR.needed_mass(0.5, Q) == int(q[Z['plateau2'] == 2.0].sum()) == 100 * 2 ** 36 and E == 1
    q, Q, E = RR.integer_mass(Z['plateau2_odd'])
    assert Q == 2 ** 37 + 3 and RR.needed_mass(0.5, Q) == int(q.max()) + 1
    lam, cnt, _Q, _E, _s = RR.member_levels(Z['plateau2_odd'], CF.FRACTIONS)
    assert lam[1] == 0.5 + 2.0 ** -36 and cnt.tolist() == [1, 3, 3, 3]
    lam, cnt, _Q, E, sets = RR.member_levels(Z['span36'], CF.FRACTIONS)
    assert E == 16 and lam[-1] == 2.0 ** -20 and cnt[-1] == 1 + 80 and (Z['span36'] > 0).sum() == 161
    assert RR.integer_mass(Z['pow2_max'])[2] == 5 and RR.integer_mass(Z['below_pow2_max'])[2] == 4
    E = RR.integer_mass(Z['tiny'])[2]
    assert 0 < math.ldexp(1.0, E - 36) < 2.0 ** -1022 and abs(Z['tiny'].max() / 1e-300 - 1) < 1e-15
    E = RR.integer_mass(Z['subnormal_max'])[2]
    assert Z['subnormal_max'].max() == 5e-320 and math.ldexp(1.0, E - 36) == 0.0 and E == -1061
    assert abs(Z['big'].max() / 1e300 - 1) < 1e-15
    lam, cnt, Q, _E, _s = RR.member_levels(Z['zero'], CF.FRACTIONS)
    assert np.isinf(lam).all() and not cnt.any() and Q == 0
    lu = Z['loguniform']
    assert 0.27 < (lu == 0).mean() < 0.33 and lu.max() / lu[lu > 0].min() > 1e39
    # the summary group
    sm = CF.summary_members(N)
    assert [w for *_x, w in sm] == list(CF.SUM_WEIGHTS) and np.array_equal(sm[0][1], sm[1][1])
    V = CF.summary_reference(N)[0]['V']
    hot = (V > 9e5).all(0)
    spread = np.ptp(V[:, hot], axis=0)
    assert hot.sum() == CF.HOT and (spread / V[0, hot] < 1e-9).all() and (spread > 0).all()


# ---- the zoo discriminates ------------------------------------------------------------------------------------------

def _peak_slot_last(h):
    m = h.max(0)
    last = h.shape[0] - 1 - np.argmax((h == m)[::-1], 0)
    return np.where(m > 0, last, h.shape[0])


def _arrival_stays(h, thr):
    """the first slot after which the value stays at or above t until the last slot"""
    out = []
    for t in thr:
        below = h < t
        last_below = h.shape[0] - 1 - np.argmax(below[::-1], 0)
        out.append(np.where(below.any(0), last_below + 1, 0))
    return np.array(out)


def _swap_pairs(f):
    g = f.ravel().copy()
    k = g.size // 2 * 2
    g[:k] = g[:k].reshape(-1, 2)[:, ::-1].ravel()
    return g.reshape(f.shape)


def _drop_tail(f):
    g = f.copy()
    g.flat[g.size - 1] = 0.0
    return g


def _bins_of(f, p):
    return np.searchsorted(EDGES, CF.history(f, p), 'right')


RULES = {      # name -> (true, altered) of one member (field, profile); the range rules take the field alone
    '> for >= at a threshold': (lambda f, p: [CF.history(f, p) >= t for t in CF.THR],
                                lambda f, p: [CF.history(f, p) > t for t in CF.THR]),
    "side='left' for 'right'": (_bins_of, lambda f, p: np.searchsorted(EDGES, CF.history(f, p), 'left')),
    'the last slot of a tie for the first': (lambda f, p: PK.peak_slot(CF.history(f, p)),
                                             lambda f, p: _peak_slot_last(CF.history(f, p))),
    'arrival: the first slot after which it stays': (lambda f, p: AR.arrival_slots(CF.history(f, p), CF.THR),
                                                     lambda f, p: _arrival_stays(CF.history(f, p), CF.THR)),
    'floor for the ceiling in needed_mass': (lambda f, p: CF.levels(f)[:2], lambda f, p: CF.levels(f, floor=True)[:2]),
    'a plateau entering partly': (lambda f, p: CF.levels(f)[:2], lambda f, p: CF.levels(f, partial=True)[:2]),
    'mass for every v > 0': (lambda f, p: CF.levels(f), lambda f, p: CF.levels(f, min_mass=1)),
    'the tail cell dropped': (_bins_of, lambda f, p: _bins_of(_drop_tail(f), p)),
    'the two cells of a pair swapped': (_bins_of, lambda f, p: _bins_of(_swap_pairs(f), p)),
    't > negval for !(t < negval)': (lambda f, p: CF.history(f, p), lambda f, p: CF.history(f, p, strict=True)),
}
RANGE_RULES = ('floor for the ceiling in needed_mass', 'a plateau entering partly', 'mass for every v > 0')


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize('N', CF.SIZES)
def test_the_zoo_discriminates_where_a_smooth_bump_does_not(N):
    Z = CF.zoo(N)
    slot_members = [(n, f, p) for n, f, p, _w in CF.members(N) if n not in ('tiny', 'subnormal_max', 'big')]
    range_fields = [(n, Z[n], None) for n in CF.RANGE_FIELDS if n != 'loguniform']
    b = CF.bump(N)
    assert b.min() > 0 and len(np.unique(b)) > N * N // 8
    bump_members = [('bump', b, p) for p in ('rising', 'falling', 'cut')]        # no slot repeats another
    blind = []
    for rule, (true, altered) in RULES.items():
        mem = range_fields if rule in RANGE_RULES else slot_members
        told_by = [n + ':' + str(p) for n, f, p in mem if not _same(true(f, p), altered(f, p))]
        assert told_by, rule
        if all(_same(true(f, p), altered(f, p)) for _n, f, p in bump_members):
            blind.append(rule)
        print('%-45s told by %3d crafted members, first %s' % (rule, len(told_by), told_by[0]))
    print('N = %d: a smooth bump cannot tell %d of %d altered rules from the true ones: %s'
          % (N, len(blind), len(RULES), blind))
    assert len(blind) >= len(RULES) - 3


# ---- the references against plain loops and exact arithmetic ----------------------------------------------------------

@pytest.mark.parametrize('N', CF.SIZES)
def test_range_levels_three_ways(N):
    for name, f, prof, w, negval in CF.range_members(N):
        for s, v in enumerate(CF.history(f, prof, negval)):
            lam, n, Q, E, sets = RR.member_levels(v, CF.FRACTIONS)
            assert (lam.tolist(), n.tolist(), Q, E) == tuple(RR.brute_levels(v, CF.FRACTIONS)), (name, s)
            if name != 'loguniform' or N == 65:
                assert (lam.tolist(), Q, E) == tuple(RR.radix_levels(v, CF.FRACTIONS)), (name, s)
            assert (lam.tolist(), n.tolist(), Q, E) == tuple(CF.levels(v)), (name, s)
            assert [int(x.sum()) for x in sets] == n.tolist()


def test_counts_equal_plain_loops():
    """histogram, arrival, peak and excursion counts of every member at N = 65, cell by cell in Python; a cell that is
    zero in every slot of every member is done once"""
    N = 65
    mem, H = CF.members(N), [h.reshape(CF.NSLOT, -1) for h in CF.histories(N)]
    weights = [w for *_x, w in mem]
    n, K, S = N * N, len(CF.THR), CF.NSLOT
    hist = HR.weighted_counts([h.T for h in H], weights, CF.EDGES)          # [B + 2, n, S]
    arr = AR.weighted_counts(H, weights, CF.THR)                              # [K, S + 1, n]
    day, dur = PK.day_counts(H, weights), PK.duration_counts(H, weights, CF.THR)
    exc = np.array([[XR.counts(XR.bits(np.array([h[s] for h in H]), t), weights) for s in range(S)] for t in CF.THR])
    live = np.flatnonzero(np.any([h.any(0) for h in H], 0))
    dead = np.setdiff1d(np.arange(n), live)
    W = sum(weights)
    assert (hist[0][dead] == W).all() and not hist[1:][:, dead].any() and (arr[:, S][:, dead] == W).all()
    assert (day[S][dead] == W).all() and (dur[:, 0][:, dead] == W).all() and not exc[:, :, dead].any()
    assert live.size > 3000
    for c in live.tolist():
        h_c = np.zeros((B + 2, S), dtype=np.int64)
        a_c = np.zeros((K, S + 1), dtype=np.int64)
        d_c, u_c = np.zeros(S + 1, dtype=np.int64), np.zeros((K, S + 1), dtype=np.int64)
        x_c = np.zeros((K, S), dtype=np.int64)
        for h, w in zip(H, weights):
            v = h[:, c].tolist()
            if not any(v):
                h_c[0] += w
                a_c[:, S] += w
                d_c[S] += w
                u_c[:, 0] += w
                continue
            best, at = 0.0, S
            for s, x in enumerate(v):
                h_c[bisect.bisect_right(CF.EDGES, x), s] += w
                if x > best:
                    best, at = x, s
            d_c[at] += w
            for k, t in enumerate(CF.THR):
                first, count = S, 0
                for s, x in enumerate(v):
                    if x >= t:
                        count += 1
                        x_c[k, s] += w
                        if first == S:
                            first = s
                a_c[k, first] += w
                u_c[k, count] += w
        assert np.array_equal(hist[:, c], h_c) and np.array_equal(arr[:, :, c], a_c), c
        assert np.array_equal(day[:, c], d_c) and np.array_equal(dur[:, :, c], u_c) and np.array_equal(exc[:, :, c], x_c), c


def test_summary_restatement_against_the_exact_moments():
    worst = {'plain': [0.0, 0.0], 'fused': [0.0, 0.0]}
    for N in CF.SIZES:
        for s, ref in enumerate(CF.summary_reference(N)):
            V = ref['V']
            for which in ('plain', 'fused'):
                mean, M2 = ref[which]
                assert (M2 >= 0).all(), (N, s, which)
                em, eq = CF.moment_errors(mean, M2, ref['exact'])
                worst[which] = [max(worst[which][0], em), max(worst[which][1], eq)]
            # two identical members: mean == v and M2 == 0 bit for bit
            mean, M2 = ref['pair']
            assert np.array_equal(mean, V[0]) and not M2.any()
            # the plain and the fused restatement are not the same thing on these members
            assert np.array_equal(ref['plain'][0], ref['fused'][0])
            if V.any():
                assert not np.array_equal(ref['plain'][1], ref['fused'][1])
    print('summary restatement vs exact moments: plain mean %.4f M2 %.4f, fused mean %.4f M2 %.4f'
          % (worst['plain'][0], worst['plain'][1], worst['fused'][0], worst['fused'][1]))
    assert CF.MEAN_ERR == MEAN_MEASURED and CF.M2_ERR == M2_MEASURED
    for which in worst:
        assert MEAN_MEASURED / 2 <= worst[which][0] <= 2 * MEAN_MEASURED
        assert M2_MEASURED / 2 <= worst[which][1] <= 2 * M2_MEASURED
    # the integer fma against the rational one, and one step by hand against the two roundings
    rng = np.random.default_rng(CF.SEED)
    for a, b, c in (10.0 ** rng.uniform(-30, 30, (2000, 3)) * rng.choice([-1.0, 1.0], (2000, 3))).tolist():
        assert CF.fma(a, b, c) == float(CF.Fraction(a) * CF.Fraction(b) + CF.Fraction(c))
        assert CF.fma(a, b, -a * b) == float(CF.Fraction(a) * CF.Fraction(b) - CF.Fraction(a * b))    # cancellation
    assert CF.fma(3.0, 1.0 / 3.0, -1.0) == -2.0 ** -54 and 3.0 * (1.0 / 3.0) - 1.0 == 0.0
