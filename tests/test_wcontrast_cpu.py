"""CPU tests of the reweighted paired contrast: the numpy restatement (wcontrast_ref) against the exact rational moments
of d on the crafted pairs under the four weight sets -- the figures of its docstring, asserted with a margin of 2 --,
against the plain two-pass definitions and, with every log-weight 0, against crafted_plans' integer reference; its
scale rule against the package's; reweighted_coverage_difference against plain numpy, against coverage_difference and
for its refusals; the 'contrast' entry of reweight's maps option, the driver tables and the script's flag."""
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import crafted_plans as CP
import wcontrast_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('N', CP.SIZES)
def test_the_restatement_against_the_exact_moments(N):
    ref, sched = WR.reference(N)
    for name in WR.NAMES:
        worst = [0.0, 0.0]
        for e in range(CP.NENTRY):
            em, eq = WR.exact_errors(ref[e][name], ref[e]['D'], sched[name][0])
            worst = [max(worst[0], em), max(worst[1], eq)]
        print('N = %d, %s: mean %.4f, M2 %.4f units' % (N, name, worst[0], worst[1]))
        assert worst[0] <= 2 * WR.MEAN_ERR[name] and worst[1] <= 2 * WR.M2_ERR[name], (name, worst)


def test_the_weight_sets_do_what_they_are_there_for():
    _ref, sched = WR.reference(65)
    steps = {n: sched[n][0] for n in WR.NAMES}
    assert all(r == 1.0 and om == w for (r, om), w in zip(steps['flat'], CP.WEIGHTS)) and sched['flat'][1] == 0.0
    rs = [r for r, _om in steps['swing']]
    assert sum(r < 1.0 for r in rs) == 2 and sched['swing'][1] == 700.5          # the reference rises twice
    assert 0.0 < steps['swing'][3][1] < 1e-200 and 0.0 < steps['swing'][5][1] < 1e-200
    assert [om > 0.0 for _r, om in steps['dead']] == [False, True, False, True, True, False]
    assert steps['under'][2] == (1.0, 0.0)                # exp(-800) underflows: skipped, and the reference stays
    assert steps['under'][4] == (0.0, 3.0) and sched['under'][1] == 800.0        # r = 0 wipes what came before
    fw = WR.final_weights(steps['under'])
    assert steps['under'][5] == (1.0, 0.0)                # and what follows at 0 underflows against the new reference
    assert fw[0] == fw[1] == fw[2] == fw[3] == fw[5] == 0 and fw[4] == 3


def test_the_scale_rule_is_the_package_s():
    from parasitoids_amd import predictive as PR
    names = list(WR.NAMES)
    refs = [-math.inf] * 4
    mine = [-math.inf] * 4
    for lam, w in zip(WR.member_lams(), CP.WEIGHTS):
        r, om, new = PR.reweight_scale(names, refs, lam, w)
        for j in range(4):
            rj, oj, nj = WR.scale(mine[j], lam[j], w)
            assert (rj, oj) == (r[j], om[j]), (lam, j)
            if oj > 0.0:
                mine[j] = nj
        refs = [b if o > 0.0 else a for a, b, o in zip(refs, new, om)]
        assert refs == mine
    for a, b in ((-math.inf, -math.inf), (0.0, -math.inf), (-math.inf, 3.0), (700.5, 0.0), (0.0, 800.0)):
        ra, rb, top = PR.reweight_merge_scale([a], [b])
        assert (ra[0], rb[0], top[0]) == WR.merge_scale(a, b)


@pytest.mark.parametrize('N', CP.SIZES[:1])
def test_the_restatement_against_the_definitions_and_the_integer_reference(N):
    ref, sched = WR.reference(N)
    plain = CP.contrast_reference(N)
    mem = CP.pair_members(N)
    Wsum = float(sum(CP.WEIGHTS))
    for e in range(CP.NENTRY):
        vals = np.array([CP.values(m, e) for m in mem])
        st = ref[e]['flat']
        # every log-weight 0: the bits of the integer reference, the sums its counts
        assert st['W'] == Wsum and np.array_equal(st['mean'], plain[e]['mom']['fused'][0])
        assert np.array_equal(st['M2'], plain[e]['mom']['fused'][1], equal_nan=True)
        for got, want in zip(st['S'], CP.contrast_count_planes(plain[e], len(CP.THR4))):
            assert np.array_equal(got, want)
        for name in WR.NAMES:
            st = ref[e][name]
            tp = WR.two_pass(vals[:, 0], vals[:, 1], WR.normalised(WR.LAM[name], CP.WEIGHTS), CP.THR4)
            tame = np.abs(ref[e]['D']).max(0) < 1e100             # the ties at 1e300: squares beyond double
            scale = np.abs(ref[e]['D'][:, tame]).max()
            np.testing.assert_allclose(WR.fetch(st, 0)[tame], tp['mean'][tame], rtol=1e-12, atol=1e-15 * scale)
            np.testing.assert_allclose(WR.fetch(st, 1)[tame], tp['var'][tame], rtol=1e-12, atol=1e-15 * scale ** 2)
            planes = [tp['pos'], tp['neg']] + [p for k in range(len(CP.THR4)) for p in (tp['gain'][k], tp['loss'][k])]
            for p, want in enumerate(planes):
                np.testing.assert_allclose(WR.fetch(st, 2 + p), want, rtol=1e-12, atol=1e-300)


def test_the_merge_of_the_restatement():
    N, e = 65, 2
    mem = CP.pair_members(N)
    vals = [CP.values(m, e) for m in mem]
    for name in WR.NAMES:
        steps_all, _ref = WR.schedule(WR.LAM[name], CP.WEIGHTS)
        halves = []
        for lo, hi in ((0, CP.HALF), (CP.HALF, 6)):
            steps, ref = WR.schedule(WR.LAM[name][lo:hi], CP.WEIGHTS[lo:hi])
            st = WR.new(N * N, 2)
            for (a, b), (r, om) in zip(vals[lo:hi], steps):
                WR.add(st, a, b, r, om, CP.THR4[:2])
            halves.append((st, ref))
        whole = WR.new(N * N, 2)
        for (a, b), (r, om) in zip(vals, steps_all):
            WR.add(whole, a, b, r, om, CP.THR4[:2])
        (sa, refa), (sb, refb) = halves
        ra, rb, top = WR.merge_scale(refa, refb)
        WR.merge(sa, sb, ra, rb)
        assert sa['members'] == whole['members'] and sa['skipped'] == whole['skipped']
        assert top + math.log(sa['W']) == pytest.approx(_ref + math.log(whole['W']), abs=1e-12)
        tame = np.abs(np.array([a - b for a, b in vals])).max(0) < 1e100
        scale = np.abs(np.array([a - b for a, b in vals])[:, tame]).max()
        np.testing.assert_allclose(WR.fetch(sa, 0)[tame], WR.fetch(whole, 0)[tame], rtol=1e-12, atol=1e-15 * scale)
        np.testing.assert_allclose(WR.fetch(sa, 1)[tame], WR.fetch(whole, 1)[tame], rtol=1e-12, atol=1e-15 * scale ** 2)
        for p in range(6):
            np.testing.assert_allclose(WR.fetch(sa, 2 + p), WR.fetch(whole, 2 + p), rtol=1e-12, atol=1e-300)
    # an empty side: a copy, or the skipped count alone
    empty, full = WR.new(N * N, 2), halves[0][0]
    WR.merge(empty, full, 1.0, 1.0)
    assert empty['W'] == full['W'] and np.array_equal(empty['M2'], full['M2'], equal_nan=True)
    before = full['mean'].copy()
    WR.merge(full, WR.new(N * N, 2), 1.0, 1.0)
    assert np.array_equal(full['mean'], before)


# ---- the covered areas under real weights ---------------------------------------------------------------------------

def _plain_area(ca, cb, w, lam, area, levels):
    """plain numpy: omega normalised, the weighted lower quantile by a sort and a cumulative sum"""
    ca, cb, w, lam = (np.asarray(x, dtype=np.float64) for x in (ca, cb, w, lam))
    alive = (w > 0) & np.isfinite(lam)
    om = np.where(alive, w * np.exp(lam - lam[alive].max()), 0.0)
    om = om / om.sum()
    out = []
    for s in range(ca.shape[1]):
        d = ca[:, s] - cb[:, s]
        order = np.argsort(d, kind='stable')
        cum = np.cumsum(om[order])
        q = [d[order][min(int(np.searchsorted(cum, p - 1e-12)), d.size - 1)] * area for p in levels]
        out.append({'mean': (om * d).sum() * area, 'quantiles': q, 'p_a_larger': om[d > 0].sum(), 'p_b_larger': om[d < 0].sum()})
    return out


def test_reweighted_coverage_difference():
    from parasitoids_amd.predictive import coverage_difference, reweighted_coverage_difference
    rng = np.random.default_rng(20261021)
    M, nout, area = 40, 3, 156.25
    ca = rng.integers(0, 500, (M, nout))
    cb = rng.integers(0, 500, (M, nout))
    cb[::7] = ca[::7]                                       # ties: neither side larger
    w = rng.integers(1, 6, M)
    levels = (0.05, 0.5, 0.95)
    # every log-weight 0 (or any one constant): coverage_difference's numbers exactly
    for const in (0.0, -700.0, 33.5):
        assert reweighted_coverage_difference(ca, cb, w, np.full(M, const), area, levels) \
            == coverage_difference(ca, cb, w, area, levels)
    # p = 1 reaches the largest d; a single member
    top = reweighted_coverage_difference(ca, cb, w, np.zeros(M), area, (1.0,))
    assert [r['quantiles'][0] for r in top] == [float((ca - cb)[:, s].max()) * area for s in range(nout)]
    for lam in (rng.normal(0.0, 3.0, M), rng.normal(0.0, 200.0, M), np.where(np.arange(M) % 3 == 0, -np.inf, rng.normal(0, 2, M))):
        got = reweighted_coverage_difference(ca, cb, w, lam, area, levels)
        want = _plain_area(ca, cb, w, lam, area, levels)
        for g, x in zip(got, want):
            assert g['mean'] == pytest.approx(x['mean'], rel=1e-12, abs=1e-9)
            assert g['quantiles'] == [pytest.approx(v) for v in x['quantiles']]
            assert g['p_a_larger'] == pytest.approx(x['p_a_larger'], rel=1e-12, abs=1e-15)
            assert g['p_b_larger'] == pytest.approx(x['p_b_larger'], rel=1e-12, abs=1e-15)
            assert 0.0 <= g['p_a_larger'] + g['p_b_larger'] <= 1.0 + 1e-15
    # members at -inf and members without weight count for nothing: the numbers of the others alone
    lam = rng.normal(0.0, 2.0, M)
    dead = np.arange(M) % 4 == 1
    lam2 = np.where(dead, -np.inf, lam)
    assert reweighted_coverage_difference(ca, cb, w, lam2, area, levels) \
        == reweighted_coverage_difference(ca[~dead], cb[~dead], w[~dead], lam[~dead], area, levels)
    # one member outweighs the rest by 300 orders of magnitude: its own difference
    lam3 = np.zeros(M)
    lam3[5] = 800.0
    one = reweighted_coverage_difference(ca, cb, w, lam3, area, levels)
    assert [r['mean'] for r in one] == [float(ca[5, s] - cb[5, s]) * area for s in range(nout)]
    # refusals
    with pytest.raises(ValueError, match='-inf'):
        reweighted_coverage_difference(ca, cb, w, np.full(M, -np.inf), area)
    with pytest.raises(ValueError, match='-inf'):
        reweighted_coverage_difference(ca, cb, np.zeros(M, dtype=int), np.zeros(M), area)
    with pytest.raises(ValueError, match='NaN'):
        reweighted_coverage_difference(ca, cb, w, np.where(np.arange(M) == 3, np.nan, 0.0), area)
    with pytest.raises(ValueError, match='NaN'):
        reweighted_coverage_difference(ca, cb, w, np.where(np.arange(M) == 3, np.inf, 0.0), area)
    with pytest.raises(ValueError, match='log-weights'):
        reweighted_coverage_difference(ca, cb, w, np.zeros(M - 1), area)
    with pytest.raises(ValueError, match='>= 0'):
        reweighted_coverage_difference(ca, cb, -w, np.zeros(M), area)


# ---- the option, the tables, the script -----------------------------------------------------------------------------

def test_the_maps_option_takes_contrast():
    from parasitoids_amd import predictive as PR
    assert PR.REWEIGHT_MAPS == ('quantiles', 'arrival', 'contrast', 'excursion')       # 'excursion' stays the last entry
    assert PR.check_reweight_maps(['excursion', 'contrast']) == ('contrast', 'excursion')
    assert PR.check_reweight_maps(['contrast', 'quantiles']) == ('quantiles', 'contrast')
    assert PR.check_reweight_maps(('contrast',)) == ('contrast',)
    with pytest.raises(ValueError, match='maps'):
        PR.check_reweight_maps(['contrast', 'contrast'])
    with pytest.raises(ValueError, match='maps'):
        PR.check_reweight_maps('contrast')
    plan = PR.check_reweight({'a': dict(log_weights=[np.zeros(4)]), 'options': dict(maps=('contrast',))})
    assert plan['maps'] == ('contrast',)


def test_the_driver_refuses_the_option_without_compare_before_any_chain():
    from parasitoids_amd import predictive as PR
    pm = types.SimpleNamespace(days=list(range(6)), rad_dist=10000.0, rad_res=64, device=None)
    rw = {'a': dict(log_weights=[np.zeros(4)]), 'options': dict(maps=('contrast',))}
    with pytest.raises(ValueError, match="maps='contrast' reweights the maps of compare=, and there is none"):
        PR.posterior_predictive(pm, object(), reweight=rw)
    with pytest.raises(ValueError, match="maps='contrast' reweights the maps of compare=, and there is none"):
        PR.posterior_predictive(pm, object(), reweight=rw, sites=dict(sites=[(0.0, 0.0, 1.0)], days=[1, 2]))


def test_the_driver_tables_and_that_nothing_is_built_without_the_option():
    from parasitoids_amd import predictive as PR
    assert PR.FEED_ORDER['compare'] == ('apply', 'contrast', 'reweight_contrast')
    for kind in ('days', 'projection', 'sites', 'ranking'):
        assert 'reweight_contrast' not in PR.FEED_ORDER[kind]
    assert 'reweight_contrast' in PR.ACCUMULATORS and PR.BUILD['reweight_contrast'] is PR._build_reweight_contrast
    assert 'reweight_contrast' in PR.FEED
    # without the option: None, and nothing is constructed (the sources are no plans: building would raise)
    fs = PR._FieldSet().fed_from('compare', object(), owns=False, against=object())
    z = np.zeros(4)
    for q in (types.SimpleNamespace(), types.SimpleNamespace(rw_plan=None),
              types.SimpleNamespace(rw_plan=PR.check_reweight({'a': dict(log_weights=[z])})),
              types.SimpleNamespace(rw_plan=PR.check_reweight({'a': dict(log_weights=[z]),
                                                               'options': dict(maps=('quantiles', 'arrival', 'excursion'))}))):
        assert PR._build_reweight_contrast(fs, q) is None
    with pytest.raises(ValueError):          # with it the class is reached, and refuses what is no pair of plans
        PR._build_reweight_contrast(fs, types.SimpleNamespace(
            thresholds=[1.0], rw_plan=PR.check_reweight({'a': dict(log_weights=[z]), 'options': dict(maps=('contrast',))})))
    res = PR.PredictiveResult(None, 0, 0, 0, 0.0, [], None, [], None)
    assert res.reweight_contrast is None and PR._FieldSet().reweight_contrast is None
    # the feed passes the run's log-weights and its length, and the set keeps them in add order
    seen = []
    acc = types.SimpleNamespace(add=lambda lam, w: seen.append((lam, w)))
    PR.FEED['reweight_contrast'](acc, None, types.SimpleNamespace(lam=[0.5, -1.0], length=3))
    assert seen == [([0.5, -1.0], 3)]


def test_the_class_checks_its_arguments_before_the_device():
    from parasitoids_amd import predictive as PR
    with pytest.raises(ValueError, match='not with itself'):
        a = object()
        PR.ReweightedContrast(a, a, ['x'])
    with pytest.raises(ValueError, match='two ReleaseSites or two Projection'):
        PR.ReweightedContrast(object(), object(), ['x'])
    assert PR.ReweightedContrast._prefix == 'ps_wcontrast'


def test_the_new_entry_points_are_declared_and_bound():
    from parasitoids_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'parasitoid_hip.h')).read()
    names = ['ps_wcontrast_' + n for n in ('create', 'add_sites', 'add_project', 'merge', 'info', 'fetch', 'reset', 'prof',
                                           'destroy')]
    for name in names:
        assert name + '(' in header and name in _lib.SIGNATURES, name
    lib = _lib.load()
    for name in names:
        assert hasattr(lib, name), name
    makefile = open(os.path.join(ROOT, 'parasitoids_amd', 'csrc', 'Makefile')).read()
    assert makefile.count('ps_wcontrast.hip') == 2            # SRCS and the file table


def test_the_script_takes_and_refuses_the_flag():
    script = os.path.join(ROOT, 'scripts', 'run_predictive.py')
    rw = ['--reweight', 'a:0,0,2,none,1e-3']
    for flags, message in ((rw + ['--reweight-maps', 'contrast'], 'give --compare-sites too'),
                           (rw + ['--reweight-maps', 'contrast,contrast', '--sites', '0,0,1', '--compare-sites', '0,0,1.5'],
                            'takes a subset'),
                           (['--reweight-maps', 'contrast', '--sites', '0,0,1', '--compare-sites', '0,0,1.5'],
                            'give --reweight or --reweight-file too')):
        r = subprocess.run([sys.executable, script, '--synthetic'] + flags, capture_output=True, text=True)
        assert r.returncode == 2 and message in r.stderr, (flags, r.stderr[-300:])
        assert 'Traceback' not in r.stderr
