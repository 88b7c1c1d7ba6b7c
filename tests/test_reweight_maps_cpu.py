"""CPU tests of the reweighted quantile and arrival maps (predictive.ReweightedHistogram / ReweightedArrival): the
numpy references whist_ref and warr_ref against the integer references they tie to, the bracket property of the
reweighted quantile under real weights, the shared weight rule, the refusals of reweight's maps option and of the
script's flag, and the driver's tables.  No device."""
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import arrival_ref as AR
import hist_ref as HR
import reweight_ref as RR
import warr_ref as WA
import whist_ref as WH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = (0.05, 0.3, 0.5, 0.95, 1.0)


def _lognormal_members(seed, members, shape, zero_share=0.3):
    rng = np.random.default_rng(seed)
    out = []
    for _m in range(members):
        v = np.exp(rng.normal(0.0, 2.5, size=shape))
        v[rng.random(shape) < zero_share] = 0.0
        out.append(v)
    return out


def test_with_all_log_weights_zero_whist_ref_is_hist_ref():
    edges = 1e-2 * 10.0 ** (np.arange(17) / 4.0)
    fields = _lognormal_members(3, 7, (2, 9, 11))
    weights = [1, 3, 1, 2, 1, 4, 2]
    st = WH.new_state((2, 9, 11), edges, 1)
    for f, w in zip(fields, weights):
        WH.add(st, f, [0.0], w)
    sc = st[0]
    assert sc['W'] == float(sum(weights)) and sc['ref'] == 0.0 and sc['members'] == 7
    counts = HR.weighted_counts(fields, weights, edges)               # [B + 2, 2, 9, 11]
    assert np.array_equal(sc['H'][1:], counts[1:].astype(np.float64)) and not sc['H'][0].any()
    for slot in range(2):
        H = sc['H'][:, slot]
        for p in LEVELS:
            b, val, lo, hi = HR.quantile_from_counts(counts[:, slot], edges, p)
            gb, gval, glo, ghi, _near = WH.quantile_from_planes(H, sc['W'], edges, p)
            assert np.array_equal(gb, b) and np.array_equal(gval, val), (slot, p)
            assert np.array_equal(glo, lo) and np.array_equal(ghi, hi), (slot, p)
        for k in (0, 5, 16):
            assert np.array_equal(WH.exceedance_from_planes(H, sc['W'], k),
                                  HR.exceedance_from_counts(counts[:, slot], k)), (slot, k)


def test_with_all_log_weights_zero_warr_ref_is_arrival_ref():
    thr = [0.5, 5.0, 50.0]
    fields = _lognormal_members(5, 6, (5, 8, 9), zero_share=0.5)
    weights = [2, 1, 1, 3, 1, 2]
    st = WA.new_state((5, 8, 9), thr, 1)
    for f, w in zip(fields, weights):
        WA.add(st, f, [0.0], w)
    sc = st[0]
    counts = AR.weighted_counts(fields, weights, thr)                 # [K, nslot + 1, 8, 9]
    assert sc['W'] == float(sum(weights))
    assert np.array_equal(sc['A'], counts[:, :-1].astype(np.float64))
    P = AR.probability(counts)
    for k in range(3):
        assert np.array_equal(WA.probability(sc['A'][k], sc['W']), P[k]), k
        for p in LEVELS:
            assert np.array_equal(WA.quantile_slots(sc['A'][k], sc['W'], p), AR.quantile_slots(counts, p)[k]), (k, p)


def test_the_bracket_holds_the_exact_reweighted_quantile():
    """The bracket [lower, upper) of the reweighted histogram holds the exact weighted lower quantile of the
    members' values.  A cell may miss it only where a running weight sits within 1e-12 W of p W -- there the two
    sums, added in different orders, may fall on either side -- and at most 1 % of the cells may."""
    edges = 1e-3 * 10.0 ** (np.arange(25) / 4.0)
    shape = (1, 40, 40)
    members = 48
    fields = _lognormal_members(11, members, shape)
    rng = np.random.default_rng(12)
    lam = rng.normal(0.0, 1.5, size=members)
    lam[5] = lam.max() + 2.0                       # a rescale late in the run
    weights = rng.integers(1, 4, size=members)
    st = WH.new_state(shape, edges, 1)
    for f, l, w in zip(fields, lam, weights):
        WH.add(st, f, [l], int(w))
    sc = st[0]
    assert sc['members'] == members and sc['ref'] == lam.max()
    real = weights * np.exp(lam - lam.max())
    assert abs(sc['W'] - real.sum()) <= 1e-12 * real.sum()
    left_out = total = 0
    for p in (0.05, 0.25, 0.5, 0.75, 0.95):
        _b, val, lo, hi, near_h = WH.quantile_from_planes(sc['H'][:, 0], sc['W'], edges, p)
        exact, _near_x = WH.exact_quantile([f[0] for f in fields], real, p)
        inside = (lo <= exact) & (exact < hi)
        assert np.all(inside | (near_h <= 1e-12)), p
        assert np.all((lo <= val) & ((val <= hi) | (hi == np.inf))), p
        left_out += int((~inside).sum())
        total += inside.size
    assert left_out <= 0.01 * total, (left_out, total)
    # the reweighting moves the quantile: not the unweighted one everywhere
    flat = WH.new_state(shape, edges, 1)
    for f, w in zip(fields, weights):
        WH.add(flat, f, [0.0], int(w))
    assert not np.array_equal(WH.quantile_from_planes(flat[0]['H'][:, 0], flat[0]['W'], edges, 0.5)[0],
                              WH.quantile_from_planes(sc['H'][:, 0], sc['W'], edges, 0.5)[0])


def test_rescale_underflow_and_a_late_start_in_the_references():
    """the log-weights of the GPU tests' scenarios: one rescale upward, the maximum again, an underflow to omega = 0,
    a scenario that starts at -inf; both references keep W, ref, members and skipped as reweight_ref does"""
    lam = {'swing': [0.0, -1.5, 2.25, 2.25, -800.0], 'late': [-math.inf, 0.5, -0.25, 3.0, 1.0]}
    weights = [1, 3, 1, 2, 1]
    fields = _lognormal_members(2, 5, (3, 6, 7))
    edges, thr = [0.1, 1.0, 10.0], [1.0, 10.0]
    h, a = WH.new_state((3, 6, 7), edges, 2), WA.new_state((3, 6, 7), thr, 2)
    s = RR.new_state((3, 6, 7), thr, 2)
    for m, (f, w) in enumerate(zip(fields, weights)):
        lams = [lam['swing'][m], lam['late'][m]]
        WH.add(h, f, lams, w)
        WA.add(a, f, lams, w)
        RR.add(s, f, lams, w)
    for j in range(2):
        for st in (h, a):
            assert [st[j][k] for k in ('W', 'ref', 'members', 'skipped')] == \
                [s[j][k] for k in ('W', 'ref', 'members', 'skipped')]
        # every member lands in at most one stored bin, and at a threshold in at most one slot
        assert np.all(WH.tails(h[j]['H'][:, 1])[1] <= h[j]['W'] * (1 + 1e-15))
        assert np.all(WA.cumulative(a[j]['A'][0])[-1] <= a[j]['W'] * (1 + 1e-15))
        # the exceedance at an edge that is a summary threshold sums the same terms as reweight_ref's S
        np.testing.assert_allclose(WH.exceedance_from_planes(h[j]['H'][:, 2], h[j]['W'], 1),
                                   RR.exceedance(s[j], 0)[2], rtol=1e-14, atol=0)
    assert [h[0]['members'], h[0]['skipped'], h[1]['members'], h[1]['skipped']] == [4, 1, 4, 1]
    # a merge of two halves lands within rounding of the whole, and into an empty state it is a copy
    h1, h2 = WH.new_state((3, 6, 7), edges, 2), WH.new_state((3, 6, 7), edges, 2)
    for m, (f, w) in enumerate(zip(fields, weights)):
        WH.add(h1 if m < 2 else h2, f, [lam['swing'][m], lam['late'][m]], w)
    empty = WH.new_state((3, 6, 7), edges, 2)
    WH.merge(empty, h2)
    assert all(np.array_equal(empty[j]['H'], h2[j]['H']) and empty[j]['W'] == h2[j]['W'] for j in range(2))
    WH.merge(h1, h2)
    for j in range(2):
        assert h1[j]['ref'] == h[j]['ref'] and h1[j]['members'] == h[j]['members']
        np.testing.assert_allclose(h1[j]['H'], h[j]['H'], rtol=1e-14, atol=0)


def test_the_weight_rule_is_one_function():
    from parasitoids_amd import predictive as PR
    names = ['a', 'b', 'c']
    refs = [-math.inf, 1.0, 2.0]
    r, om, ref = PR.reweight_scale(names, refs, [0.5, 3.0, -800.0], 2)
    want = [RR.scale(x, l, 2) for x, l in zip(refs, [0.5, 3.0, -800.0])]
    assert list(zip(r, om, ref)) == want and om[2] == 0.0
    assert PR.reweight_scale(names, refs, {'c': 0.0, 'a': -math.inf, 'b': 1.0}) == \
        ([1.0, 1.0, 1.0], [0.0, 1.0, math.exp(-2.0)], refs)
    for bad in ([0.0, math.nan, 0.0], [math.inf, 0.0, 0.0], [0.0, 0.0], 'abc', {'a': 0.0}):
        with pytest.raises(ValueError):
            PR.reweight_scale(names, refs, bad)
    for w in (0, -1, math.nan, math.inf):
        with pytest.raises(ValueError, match='weight'):
            PR.reweight_scale(names, refs, [0.0, 0.0, 0.0], w)
    assert PR.reweight_merge_scale([-math.inf, 0.0, 2.0], [-math.inf, 1.0, -math.inf]) == \
        ([1.0, math.exp(-1.0), 1.0], [1.0, 1.0, 0.0], [-math.inf, 1.0, 2.0])
    # all three classes go through it
    import inspect
    for cls in (PR.ReweightedSummary, PR._ReweightedCounts):
        assert 'reweight_scale(' in inspect.getsource(cls.scale)
    assert issubclass(PR.ReweightedHistogram, PR._ReweightedCounts)
    assert issubclass(PR.ReweightedArrival, PR._ReweightedCounts)
    # real weights in weighted_lower_quantile; integer ones as before
    assert PR.weighted_lower_quantile([3, 1, 2], [0.2, 0.5, 0.3], 0.6) == 2
    assert PR.weighted_lower_quantile([3, 1, 2], [1, 1, 1], 0.6) == 2
    assert PR.weighted_lower_quantile([3, 1, 2], [0.0, 1e-300, 0.0], 0.99) == 1


def test_the_weighted_quantile_with_real_weights_against_its_definition():
    """min{a : sum of w_m over a_m <= a >= p W} with real weights, against an expectation that shares nothing with
    the function: at p = 1 the largest value among the members with weight > 0, whatever the order in which W was
    summed (the total by pairwise summation and the running sum differ by an ulp in about a third of the draws); at
    other levels a loop in exact rational arithmetic, on draws where no running weight ties p W"""
    from fractions import Fraction
    from parasitoids_amd import predictive as PR
    off_by_an_ulp = 0
    for seed in range(200):
        rng = np.random.default_rng(seed)
        n = rng.integers(1, 4, size=40)
        w = n * np.exp(rng.normal(0.0, 1.5, size=40))
        w[rng.integers(0, 40, size=5)] = 0.0                   # members without weight: lambda = -inf
        values = rng.integers(0, 5000, size=40)
        off_by_an_ulp += int(np.cumsum(w[np.argsort(values, kind='stable')])[-1] != w.sum())
        assert PR.weighted_lower_quantile(values, w, 1.0) == values[w > 0].max(), seed
        exact = [(int(v), Fraction(float(x))) for v, x in zip(values, w)]
        W = sum(x for _v, x in exact)
        for p in (0.05, 0.5, 0.95):
            want = min(a for a, _x in exact if sum(x for v, x in exact if v <= a) >= Fraction(p) * W)
            assert PR.weighted_lower_quantile(values, w, p) == want, (seed, p)
    assert off_by_an_ulp > 20                                    # the case the comparison against w.sum() got wrong
    # integer weights: as before, against the same definition
    assert PR.weighted_lower_quantile([5, 1, 3, 1], [1, 2, 1, 1], 1.0) == 5
    assert PR.weighted_lower_quantile([5, 1, 3, 1], [1, 2, 1, 1], 0.6) == 1
    assert PR.weighted_lower_quantile([5, 1, 3, 1], [1, 2, 1, 1], 0.61) == 3


def test_the_maps_option_is_checked_before_any_evaluation():
    from parasitoids_amd import predictive as PR
    z = np.zeros(4)
    base = {'a': dict(log_weights=[z])}
    assert 'maps' not in PR.check_reweight(base)
    assert 'maps' not in PR.check_reweight(dict(base, options=dict(min_ess=5)))
    assert 'maps' not in PR.check_reweight(dict(base, options=dict(maps=())))
    assert PR.check_reweight(dict(base, options=dict(maps=['arrival', 'quantiles'])))['maps'] == ('quantiles', 'arrival')
    assert PR.check_reweight(dict(base, options=dict(maps=('arrival',), min_ess=5)))['maps'] == ('arrival',)
    for bad in ('quantiles', ['peak'], ['quantiles', 'quantiles'], ['quantiles', 'histogram'], 3):
        with pytest.raises(ValueError, match='maps'):
            PR.check_reweight(dict(base, options=dict(maps=bad)))
    with pytest.raises(ValueError, match='options'):
        PR.check_reweight(dict(base, options=dict(map=('arrival',))))
    # the driver: refused with the arguments alone, before a chain is loaded or a model touched
    pm = types.SimpleNamespace(days=list(range(6)), rad_dist=10000.0, rad_res=64, device=None)
    chains = object()                    # never looked at
    both = dict(base, options=dict(maps=('quantiles', 'arrival')))
    with pytest.raises(ValueError, match="maps='quantiles'"):
        PR.posterior_predictive(pm, chains, reweight=both, arrival=[1.0])
    with pytest.raises(ValueError, match="maps='arrival'"):
        PR.posterior_predictive(pm, chains, reweight=both, quantiles=[0.5])
    with pytest.raises(ValueError, match='not a subset'):
        PR.posterior_predictive(pm, chains, reweight=dict(base, options=dict(maps=('peak',))), quantiles=[0.5])


def test_the_script_refuses_a_bad_reweight_maps_flag():
    """refused by the argument parser, before the package is imported"""
    script = os.path.join(ROOT, 'scripts', 'run_predictive.py')
    rw = ['--reweight', 'a:0,0,1,none,1']
    for flags, message in (
            (['--reweight-maps', 'quantiles', '--quantiles', '0.5'], 'give --reweight or --reweight-file too'),
            (rw + ['--reweight-maps', 'quantiles,peak', '--quantiles', '0.5'], 'takes a subset'),
            (rw + ['--reweight-maps', 'arrival,arrival', '--arrival', '1'], 'takes a subset'),
            (rw + ['--reweight-maps', 'quantiles'], 'give --quantiles too'),
            (rw + ['--reweight-maps', 'quantiles,arrival', '--quantiles', '0.5'], 'give --arrival too')):
        r = subprocess.run([sys.executable, script, '--synthetic'] + flags, capture_output=True, text=True)
        assert r.returncode == 2 and message in r.stderr, (flags, r.stderr[-300:])
        assert 'Traceback' not in r.stderr


def test_the_driver_tables_and_that_nothing_is_built_without_the_option():
    from parasitoids_amd import predictive as PR
    new = ('reweight_histogram', 'reweight_arrival')
    for name in new:
        assert name in PR.ACCUMULATORS and name in PR.BUILD and name in PR.FEED
    for kind in ('days', 'sites'):
        order = PR.FEED_ORDER[kind]
        assert order.index('reweight') < order.index('reweight_histogram') < order.index('reweight_arrival') \
            < order.index('modes')
        assert order[-1] == 'modes'
    order = PR.FEED_ORDER['projection']
    assert order.index('reweight') < order.index('reweight_histogram') and 'reweight_arrival' not in order
    assert not set(new) & set(PR.FEED_ORDER['compare'])
    # the placements the earlier maps rest on
    days = PR.FEED_ORDER['days']
    assert days.index('origin') == days.index('summary') + 1
    for kind in ('days', 'projection', 'sites'):
        order = PR.FEED_ORDER[kind]
        assert order.index('dependence') == order.index('sensitivity') + 1
    for kind in ('days', 'sites'):
        order = PR.FEED_ORDER[kind]
        assert order.index('pathways') > order.index('patches')
        assert order.index('proximity') > order.index('neighbourhood')
    # without maps: None, and nothing is constructed (the source is not a model: building would raise)
    fs = PR._FieldSet().fed_from('days', object(), owns=False)
    z = np.zeros(4)
    for q in (types.SimpleNamespace(), types.SimpleNamespace(rw_plan=None),
              types.SimpleNamespace(rw_plan=PR.check_reweight({'a': dict(log_weights=[z])})),
              types.SimpleNamespace(rw_plan=PR.check_reweight({'a': dict(log_weights=[z]), 'options': dict(min_ess=1)}))):
        for name in new:
            assert PR.BUILD[name](fs, q) is None and getattr(fs, name) is None
    # with it the builder does go for the class
    q = types.SimpleNamespace(rw_plan=PR.check_reweight({'a': dict(log_weights=[z]), 'options': dict(maps=['arrival'])}),
                              a_thr=[1.0], bins=PR.DEFAULT_BINS, edges=None)
    assert PR.BUILD['reweight_histogram'](fs, q) is None
    with pytest.raises(AttributeError):
        PR.BUILD['reweight_arrival'](fs, q)          # object() has no days: the constructor was entered
    pr = PR.ProjectedMaps(None, None, None, None)
    res = PR.PredictiveResult(None, 0, 0, 0, 0.0, [], None, [], None)
    for name in new:
        assert getattr(pr, name) is None and getattr(res, name) is None


def test_the_new_entry_points_are_declared_and_bound():
    from parasitoids_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'parasitoid_hip.h')).read()
    common = ('create', 'add', 'add_project', 'add_sites', 'merge', 'info', 'quantile', 'fetch', 'reset', 'prof',
              'destroy')
    for prefix, own in (('ps_whist_', ('exceed',)), ('ps_warr_', ('prob',))):
        for n in common + own:
            assert prefix + n in _lib.SIGNATURES and prefix + n + '(' in header, prefix + n
    makefile = open(os.path.join(ROOT, 'parasitoids_amd', 'csrc', 'Makefile')).read()
    assert ' ps_whist.hip ' in makefile and ' ps_warr.hip ' in makefile
