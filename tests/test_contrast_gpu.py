"""GPU tests of the paired contrast of two plans (ps_contrast_*, predictive.PlanContrast): the device's mean,
count planes and coverage rows bit for bit against the numpy replay (contrast_ref) of the two plans' fetched
fields, the variance within the tolerances of the SpreadSummary tests; antisymmetry, identical plans, the tie to
SpreadSummary (half a plan; gain - loss against the two summaries' exceedance counts), weights, merges and reset,
the untouched accumulators beside it, a pair of projections, posterior_predictive with compare=, the refusals of
the C ABI, and the grid-stride path at R = 768.  Kalbar wind, R = 64 (N = 129: odd, so the tail cell and the
pairs that straddle a row end exist), 6 days, the members, weights and plans of test_sites_gpu.py."""
import ctypes as C
import json
import os
import types
import warnings

import numpy as np
import pytest

import contrast_ref
from test_sites_gpu import MEMBERS, STAGGERED, WEIGHTS, _chain, _csr, _edge_plan, _evaluate, _metres, _pop_model

pytestmark = pytest.mark.gpu

R, N = 64, 129
THR = [1.0, 10.0]
DAYS = list(range(6))
OUT = [0, 1, 2, 3, 5]
PLAN_A = STAGGERED                                                       # a group released two days later
PLAN_B = [(dr, dc, 0.75 * a, lag) for dr, dc, a, lag in _edge_plan(R)]     # scaled: either side wins somewhere
PLAN_HALF = [(dr, dc, 0.5 * a, lag) for dr, dc, a, lag in STAGGERED]


def _replay(fa, fb, weights, thr, members=None):
    """per output the contrast_ref state over the members' fields fa, fb [member][output]"""
    idx = range(len(weights)) if members is None else members
    states = []
    for e in range(len(fa[0])):
        st = contrast_ref.new_state(fa[0][e].shape, thr)
        for i in idx:
            contrast_ref.add(st, fa[i][e], fb[i][e], weights[i])
        states.append(st)
    return states


def _check_exact(X, states, nout):
    """mean, every count plane and every coverage row of X against the replay, bit for bit"""
    nthr = len(X.thresholds)
    for e in range(nout):
        st = states[e]
        assert np.array_equal(X.mean(e), st['mean']), (e, np.abs(X.mean(e) - st['mean']).max())
        for which, plane in enumerate(contrast_ref.planes(st)):
            got = X.counts(e, which)
            assert got.dtype == np.uint32 and np.array_equal(got.astype(np.int64), plane), (e, which)
    for k in range(nthr):
        ca, cb, w = X.coverage(k)
        assert ca.dtype == np.int64 and ca.shape == (len(states[0]['weights']), nout)
        assert list(w) == states[0]['weights']
        for e in range(nout):
            assert list(ca[:, e]) == [r[k] for r in states[e]['cells_a']], (k, e)
            assert list(cb[:, e]) == [r[k] for r in states[e]['cells_b']], (k, e)


def _check_variance(X, fa, fb, weights, nout):
    """against a numpy two-pass, the tolerances of test_predictive_gpu._check: rtol 1e-12, atol 1e-15 scale^2"""
    for e in range(nout):
        d = np.array([np.asarray(a[e]) - np.asarray(b[e]) for a, b in zip(fa, fb)])
        _mean, var = contrast_ref.two_pass(d, weights)
        scale = np.abs(d).max()
        got = X.variance(e)
        print('variance, output %d: max abs error %.3g, scale^2 %.3g' % (e, np.abs(got - var).max(), scale ** 2))
        np.testing.assert_allclose(got, var, rtol=1e-12, atol=1e-12 * 1e-3 * scale ** 2)


@pytest.fixture(scope='module')
def fed():
    """plan A (staggered), plan B (the edge plan), half of A and a twin of A applied to the five members, every
    accumulator the tests read fed alongside, the fields fetched, and the replay computed once"""
    from parasitoids_amd.predictive import (ArrivalMaps, PlanContrast, ReleaseSites, SpreadHistogram, SpreadSummary,
                                            lagged_models)
    pm = _pop_model(R)
    late = lagged_models(pm, [2])
    A = ReleaseSites(pm, _metres(PLAN_A, R), OUT, late)
    A2 = ReleaseSites(pm, _metres(PLAN_A, R), OUT, late)
    B = ReleaseSites(pm, _metres(PLAN_B, R), OUT)
    Hf = ReleaseSites(pm, _metres(PLAN_HALF, R), OUT, late)
    f = types.SimpleNamespace(pm=pm, late=late, A=A, A2=A2, B=B, Hf=Hf)
    f.X = PlanContrast(A, B, THR)
    f.Xr = PlanContrast(B, A, THR)
    f.Xsame = PlanContrast(A, A2, THR)
    f.Xhalf = PlanContrast(A, Hf, THR)
    f.X0 = PlanContrast(A, B)                               # no thresholds: the sign counts alone, no rows
    f.Xunit = PlanContrast(A, B, THR)
    f.Xlo, f.Xhi = PlanContrast(A, B, THR), PlanContrast(A, B, THR)
    f.S, f.SB = SpreadSummary.for_projection(A, THR), SpreadSummary.for_projection(B, THR)
    f.H, f.Arr = SpreadHistogram.for_projection(A), ArrivalMaps.for_projection(A, THR)
    f.fa, f.fb = [], []
    for i, (mem, w) in enumerate(zip(MEMBERS, WEIGHTS)):
        _evaluate(pm, mem)
        _evaluate(late[2], mem, ndays=4)
        A.apply()
        for acc in (f.S, f.H, f.Arr):
            acc.add(w)
        for plan in (B, A2, Hf):
            plan.apply()
        f.SB.add(w)
        for acc in (f.X, f.Xr, f.Xsame, f.Xhalf, f.X0, f.Xlo if i < 2 else f.Xhi):
            acc.add(w)
        for _ in range(w):
            f.Xunit.add(1)
        f.fa.append([A.field(e) for e in range(len(OUT))])
        f.fb.append([B.field(e) for e in range(len(OUT))])
    f.ref = _replay(f.fa, f.fb, WEIGHTS, THR)
    yield f
    for h in (f.X, f.Xr, f.Xsame, f.Xhalf, f.X0, f.Xunit, f.Xlo, f.Xhi, f.S, f.SB, f.H, f.Arr, A, A2, B, Hf, pm, late[2]):
        h.close()


def test_against_the_reference_bit_for_bit(fed):
    X, ref = fed.X, fed.ref
    assert X.N == N and X.nout == 5 and X.labels == OUT and X.live == list(range(5)) and X.thresholds == THR
    assert X.total_weight == sum(WEIGHTS) and X.members == len(MEMBERS)
    assert X.nbytes == 5 * ((N * N + 63) // 64 * 64) * (16 + 4 * 6) and X.cell_area == (10000.0 / R) ** 2
    # the inputs can fail: both signs, a gain and a loss at each threshold, something at the tail cell's row or
    # column, and coverage rows that tell the plans apart
    d = np.array(fed.fa) - np.array(fed.fb)
    assert (d > 0).any() and (d < 0).any()
    for k in range(len(THR)):
        assert max(st['gain'][k].max() for st in ref) > 0 and max(st['loss'][k].max() for st in ref) > 0
    assert d[:, :, N - 1, N - 1].any() or d[:, :, N - 1, :].any() or d[:, :, :, N - 1].any()
    assert any(st['cells_a'] != st['cells_b'] for st in ref)
    assert all(0 < st['pos'].max() <= sum(WEIGHTS) and 0 < st['neg'].max() for st in ref[2:])
    _check_exact(X, ref, 5)
    _check_variance(X, fed.fa, fed.fb, WEIGHTS, 5)
    W = float(sum(WEIGHTS))
    assert np.array_equal(X.prob_positive(2), ref[2]['pos'] / W) and np.array_equal(X.prob_negative(2), ref[2]['neg'] / W)
    assert np.array_equal(X.gain(4, 1), ref[4]['gain'][1] / W) and np.array_equal(X.loss(4, 0), ref[4]['loss'][0] / W)
    assert np.array_equal(X.sd(3), np.sqrt(X.variance(3))) and list(X.weights) == WEIGHTS
    # without thresholds: the same moments and sign counts, no gain / loss planes and no rows
    X0 = fed.X0
    assert X0.nbytes == 5 * ((N * N + 63) // 64 * 64) * (16 + 4 * 2) and list(X0.weights) == WEIGHTS
    for e in range(5):
        assert np.array_equal(X0.mean(e), X.mean(e)) and np.array_equal(X0.variance(e), X.variance(e))
        assert np.array_equal(X0.counts(e, 0), X.counts(e, 0)) and np.array_equal(X0.counts(e, 1), X.counts(e, 1))
    with pytest.raises(ValueError):
        X0.counts(0, 2)
    with pytest.raises(ValueError):
        X0.coverage(0)
    diff = X.coverage_difference(1, (0.5,))
    ca, cb, w = X.coverage(1)
    from parasitoids_amd.predictive import coverage_difference
    assert [r['label'] for r in diff] == OUT
    assert [{k: v for k, v in r.items() if k != 'label'} for r in diff] == coverage_difference(ca, cb, w, X.cell_area, (0.5,))


def test_antisymmetry(fed):
    X, Xr = fed.X, fed.Xr
    for e in range(5):
        assert np.array_equal(Xr.mean(e), -X.mean(e)) and np.abs(X.mean(e)).max() > 0
        assert np.array_equal(Xr.variance(e), X.variance(e))
        for k in range(3):
            assert np.array_equal(Xr.counts(e, 2 * k), X.counts(e, 2 * k + 1))
            assert np.array_equal(Xr.counts(e, 2 * k + 1), X.counts(e, 2 * k))
    for k in range(2):
        ca, cb, w = X.coverage(k)
        ra, rb, rw = Xr.coverage(k)
        assert np.array_equal(ra, cb) and np.array_equal(rb, ca) and np.array_equal(rw, w)


def test_identical_plans_leave_everything_zero(fed):
    X = fed.Xsame
    assert X.members == len(MEMBERS) and X.total_weight == sum(WEIGHTS)
    for e in range(5):
        assert not X.mean(e).any() and not X.variance(e).any()
        for which in range(6):
            assert not X.counts(e, which).any()
    for k in range(2):
        ca, cb, _w = X.coverage(k)
        assert np.array_equal(ca, cb) and ca.min() > 0
        assert np.array_equal(ca, fed.X.coverage(k)[0])


def test_tie_to_the_spread_summary(fed):
    """B = A with every amount halved: d = a / 2 exactly, so the contrast is the summary of A scaled by powers of
    two; and for any pair of plans gain - loss is the difference of the two summaries' exceedance counts"""
    W = fed.S.total_weight
    for e in range(5):
        assert np.array_equal(fed.Xhalf.mean(e), 0.5 * fed.S.mean(e)) and fed.S.mean(e).max() > 0
        assert np.array_equal(fed.Xhalf.variance(e), 0.25 * fed.S.variance(e)) and fed.S.variance(e).max() > 0
        assert not fed.Xhalf.counts(e, 1).any()
        for k in range(2):
            na = np.rint(fed.S.exceedance(e, k) * W).astype(np.int64)
            nb = np.rint(fed.SB.exceedance(e, k) * W).astype(np.int64)
            net = fed.X.counts(e, 2 + 2 * k).astype(np.int64) - fed.X.counts(e, 3 + 2 * k).astype(np.int64)
            assert np.array_equal(net, na - nb) and (na != nb).any()


def test_weights_merges_and_reset(fed):
    from parasitoids_amd.predictive import PlanContrast
    X, U, lo, hi = fed.X, fed.Xunit, fed.Xlo, fed.Xhi
    # weight w against w unit adds: the tolerances of test_weight_three_equals_three_unit_adds
    assert U.total_weight == X.total_weight and U.members == sum(WEIGHTS)
    for e in range(5):
        ma = X.mean(e)
        np.testing.assert_allclose(U.mean(e), ma, rtol=1e-13, atol=1e-16 * np.abs(ma).max())
        np.testing.assert_allclose(U.variance(e), X.variance(e), rtol=1e-13, atol=1e-13 * 1e-3 * np.abs(ma).max() ** 2)
        for which in range(6):
            assert np.array_equal(U.counts(e, which), X.counts(e, which))
    ca, _cb, w = U.coverage(0)
    assert list(w) == [1] * sum(WEIGHTS) and np.array_equal(ca, np.repeat(X.coverage(0)[0], WEIGHTS, axis=0))
    # two handles merged against one over all members: the tolerances of test_merge_equals_one_summary_over_all_members
    lo.merge(hi)
    assert lo.total_weight == X.total_weight and lo.members == X.members and hi.members == 3
    for e in range(5):
        m = X.mean(e)
        np.testing.assert_allclose(lo.mean(e), m, rtol=1e-12, atol=1e-15 * np.abs(m).max())
        np.testing.assert_allclose(lo.variance(e), X.variance(e), rtol=1e-12, atol=1e-15 * np.abs(m).max() ** 2)
        for which in range(6):
            assert np.array_equal(lo.counts(e, which), X.counts(e, which))
    for k in range(2):
        for got, want in zip(lo.coverage(k), X.coverage(k)):
            assert np.array_equal(got, want)                 # the rows in add order, hi's after lo's
    # into an empty handle: a copy, bit for bit; then reset
    with PlanContrast(fed.A, fed.B, THR) as E:
        E.merge(X)
        assert E.members == X.members and E.total_weight == X.total_weight
        for e in range(5):
            assert np.array_equal(E.mean(e), X.mean(e)) and np.array_equal(E.variance(e), X.variance(e))
            for which in range(6):
                assert np.array_equal(E.counts(e, which), X.counts(e, which))
        for k in range(2):
            for got, want in zip(E.coverage(k), X.coverage(k)):
                assert np.array_equal(got, want)
        E.reset()
        assert E.members == 0 and E.total_weight == 0 and E.coverage(0)[0].shape == (0, 5)
        E.merge(hi)
        ref = _replay(fed.fa, fed.fb, WEIGHTS, THR, members=[2, 3, 4])
        _check_exact(E, ref, 5)
        with pytest.raises(ValueError, match='different outputs'):
            E.merge(types.SimpleNamespace(live=[0], nout=1, labels=[0]))


def test_the_accumulators_beside_a_contrast_are_untouched(fed):
    """plan A's summary, histogram and arrival maps filled alone, from fresh models (an auto-mode model routes
    days by what it has seen before), against those filled beside the contrasts"""
    from parasitoids_amd.predictive import ArrivalMaps, ReleaseSites, SpreadHistogram, SpreadSummary
    pm = _pop_model(R)
    with ReleaseSites.with_lagged_models(pm, _metres(PLAN_A, R), OUT) as A, SpreadSummary.for_projection(A, THR) as S, \
            SpreadHistogram.for_projection(A) as H, ArrivalMaps.for_projection(A, THR) as Arr:
        for mem, w in zip(MEMBERS, WEIGHTS):
            _evaluate(pm, mem)
            _evaluate(A.lagged[2], mem, ndays=4)
            A.apply()
            for acc in (S, H, Arr):
                acc.add(w)
        for e, day in enumerate(OUT):
            assert np.array_equal(S.mean(e), fed.S.mean(e)) and np.array_equal(S.variance(e), fed.S.variance(e))
            assert np.array_equal(H.counts(e), fed.H.counts(e))
            for k in range(2):
                assert np.array_equal(S.exceedance(e, k), fed.S.exceedance(e, k))
                assert np.array_equal(Arr.counts(k, day), fed.Arr.counts(k, day))
        for k in range(2):
            assert np.array_equal(Arr.reached(k)[0], fed.Arr.reached(k)[0])
    pm.close()


def test_a_pair_of_projections():
    from parasitoids_amd.predictive import PlanContrast, Projection, ReleaseSites, exposure_weights
    pm = _pop_model(R)
    zero = np.zeros((1, 6))
    Wa = np.concatenate([exposure_weights(DAYS, [0, 2]), zero, exposure_weights(DAYS, [5])])
    Wb = np.concatenate([exposure_weights(DAYS, [1, 3]), zero, exposure_weights(DAYS, [4])])
    thr = [50.0, 500.0]
    fa, fb = [], []
    with Projection(pm, Wa, DAYS) as PA, Projection(pm, Wb, DAYS) as PB, PlanContrast(PA, PB, thr) as X, \
            ReleaseSites(pm, [(0, 0, 1.0)], [0, 1, 2, 3]) as RS:
        assert X.live == [0, 1, 3] and X.nout == 4 and X.labels == [0, 1, 2, 3]
        with pytest.raises(ValueError, match='two ReleaseSites or two Projection'):
            PlanContrast(PA, RS)
        with pytest.raises(ValueError, match='not with itself'):
            PlanContrast(PA, PA)
        with Projection(pm, Wa[:2], DAYS) as short, pytest.raises(ValueError, match='differ in nout'):
            PlanContrast(PA, short)
        with ReleaseSites(pm, [(0, 0, 0.5)], [0, 1, 2, 5]) as other, pytest.raises(ValueError, match='differ in days'):
            PlanContrast(RS, other)                        # as many outputs, other days: not paired by index
        for mem, w in zip(MEMBERS[:3], WEIGHTS[:3]):
            _evaluate(pm, mem)
            PA.apply()
            PB.apply()
            X.add(w)
            fa.append([PA.field(e) for e in range(4)])
            fb.append([PB.field(e) for e in range(4)])
        ref = _replay(fa, fb, WEIGHTS[:3], thr)
        # up to day 0 against up to day 1: B ahead everywhere; up to day 5 against up to day 4: A ahead
        assert ref[0]['neg'].max() == 5 and not ref[0]['pos'].any() and ref[3]['pos'].max() == 5
        assert ref[0]['loss'][1].max() > 0
        assert not fa[0][2].any() and not ref[2]['mean'].any() and ref[2]['cells_a'] == [[0, 0]] * 3
        _check_exact(X, ref, 4)
        _check_variance(X, fa, fb, WEIGHTS[:3], 4)
    pm.close()


def test_posterior_predictive_with_a_compared_plan(tmp_path, monkeypatch):
    from parasitoids_amd import mcmc
    from parasitoids_amd import predictive as PR
    trace, names = _chain([2, 1, 3, 1, 2])
    chains = [(trace[:5], names), (trace[5:], names)]
    plan_b = [(0, 0, 1.5, 0), (-5, 3, 0.5, 2), (7, -4, 0.25, 3)]

    def as_arg(cells):
        return [s[:3] + ((s[3],) if s[3] else ()) for s in _metres(cells, R)]
    arg = dict(sites=as_arg(STAGGERED), days=OUT)
    cmp_arg = dict(sites=as_arg(plan_b))
    kw = dict(thresholds=THR, arrival=THR, arrival_levels=(0.5,))
    # count the evaluations of every model of the union of the plans' later release days
    real = PR.lagged_models
    made_for, calls = [], {}

    def counting(pop_model, lags, wind_data=None):
        made = real(pop_model, lags, wind_data)
        made_for.append((pop_model, sorted(made)))
        for lag, m in made.items():
            def evaluate(*a, _inner=m.evaluate, _key=(id(pop_model), lag), **k):
                calls[_key] = calls.get(_key, 0) + 1
                return _inner(*a, **k)
            m.evaluate = evaluate
        return made
    monkeypatch.setattr(PR, 'lagged_models', counting)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        pa, pb, pc, pd = (_pop_model(R, mode='exact') for _ in range(4))
        res = PR.posterior_predictive(pa, chains, sites=arg, compare=cmp_arg, **kw)
        assert made_for == [(pa, [2, 3])] and calls == {(id(pa), 2): 6, (id(pa), 3): 6}
        par = PR.posterior_predictive([pb, pc], chains, sites=arg, compare=cmp_arg, **kw)
        assert [m for _p, m in made_for[1:]] == [[2, 3], [2, 3]] and {p for p, _m in made_for[1:]} == {pb, pc}
        assert all(calls[(id(p), lag)] == 3 for p in (pb, pc) for lag in (2, 3))
        plain = PR.posterior_predictive(pd, chains, sites=arg, **kw)
    monkeypatch.setattr(PR, 'lagged_models', real)
    X = res.contrast
    assert plain.contrast is None and plain.compare_plan is None and res.failed == 0 and len(res.runs) == 6
    assert X.total_weight == 9 and X.members == 6 and X.labels == OUT and X.thresholds == THR
    assert res.compare_plan['lags'] == [0, 2, 3] and res.compare_plan['days'] == OUT
    assert [(s['drow'], s['dcol'], s['amount'], s['lag']) for s in res.compare_plan['sites']] == plan_b
    # plan A's own maps do not know about the comparison
    for e in range(5):
        assert np.array_equal(res.sites.summary.mean(e), plain.sites.summary.mean(e))
        assert np.array_equal(res.sites.summary.variance(e), plain.sites.summary.variance(e))
        assert np.array_equal(res.sites.arrival.counts(1, OUT[e]), plain.sites.arrival.counts(1, OUT[e]))
    # by hand: one contrast per chain, merged in chain order
    cols = [names.index(m[0]) for m in mcmc.MODEL_BLOCK]
    pm = _pop_model(R, mode='exact')
    late = real(pm, [2, 3])
    fa, fb, wts = [], [], []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        with PR.ReleaseSites(pm, arg['sites'], OUT, late) as A, PR.ReleaseSites(pm, cmp_arg['sites'], OUT, late) as B, \
                PR.PlanContrast(A, B, THR) as M0, PR.PlanContrast(A, B, THR) as M1:
            for ci, first, weight in res.runs:
                args = mcmc.model_args(chains[ci][0][first, cols])
                pm.evaluate(*args, want_stats=False)
                for lag, m in sorted(late.items()):
                    m.evaluate(*args, ndays=OUT[-1] - lag + 1, want_stats=False)
                A.apply()
                B.apply()
                (M0, M1)[ci].add(weight)
                fa.append([A.field(e) for e in range(5)])
                fb.append([B.field(e) for e in range(5)])
                wts.append(weight)
            M0.merge(M1)
            ref = _replay(fa, fb, wts, THR)
            assert max(st['gain'][1].max() for st in ref) > 0 and max(st['loss'][1].max() for st in ref) > 0
            for got in (X, par.contrast, M0):
                for e in range(5):
                    m = M0.mean(e)
                    if got is not M0:
                        # the same adds per chain and the same merge in chain order, in exact mode, from fresh
                        # models per path: the driver, sequential or parallel, equals the manual loop bit for bit
                        assert np.array_equal(got.mean(e), m), e
                        assert np.array_equal(got.variance(e), M0.variance(e)), e
                    # the unmerged replay over all six members: the merge re-associates (the summary's
                    # tolerance for a merge against one accumulation, test_merge_equals_one_summary_over_all_members)
                    np.testing.assert_allclose(got.mean(e), ref[e]['mean'], rtol=1e-12, atol=1e-15 * np.abs(m).max())
                    for which, plane in enumerate(contrast_ref.planes(ref[e])):
                        assert np.array_equal(got.counts(e, which).astype(np.int64), plane), (e, which)
                for k in range(2):
                    ca, cb, w = got.coverage(k)
                    assert list(w) == wts
                    assert np.array_equal(ca, np.array([[r[k] for r in st['cells_a']] for st in ref]).T)
                    assert np.array_equal(cb, np.array([[r[k] for r in st['cells_b']] for st in ref]).T)
    # the result files
    npz, js = res.save(str(tmp_path / 'a' / 'pp'))
    plain.save(str(tmp_path / 'p' / 'pp'))
    assert not os.path.exists(str(tmp_path / 'p' / 'pp_contrast.npz'))
    for name in ('pp.npz', 'pp_sites.npz'):                # the other files do not know about the comparison
        with np.load(str(tmp_path / 'a' / name)) as fx, np.load(str(tmp_path / 'p' / name)) as fp:
            assert set(fx.files) == set(fp.files)
            for key in fp.files:
                assert np.array_equal(fx[key], fp[key]), key
    with np.load(str(tmp_path / 'a' / 'pp_contrast.npz')) as fz:
        assert [int(x) for x in fz['days']] == OUT
        want = {'days', 'contrast_weights', 'coverage0_a', 'coverage0_b', 'coverage1_a', 'coverage1_b'}
        for e, lab in enumerate(OUT):
            for suffix, m in (('', X.mean(e)), ('_sd', X.sd(e)), ('_ppos', X.prob_positive(e)),
                              ('_pneg', X.prob_negative(e)), ('_pgain0', X.gain(e, 0)), ('_ploss0', X.loss(e, 0)),
                              ('_pgain1', X.gain(e, 1)), ('_ploss1', X.loss(e, 1))):
                assert np.array_equal(_csr(fz, '%d%s' % (lab, suffix), N), np.where(np.abs(m) >= 1e-8, m, 0.0)), (lab, suffix)
                want |= {'%d%s_%s' % (lab, suffix, t) for t in ('data', 'ind', 'indptr')}
        assert set(fz.files) == want
        assert (_csr(fz, '5', N) < 0).any() and (_csr(fz, '5', N) > 0).any()       # the signed mean keeps both signs
        assert np.array_equal(fz['coverage1_a'], X.coverage(1)[0]) and np.array_equal(fz['coverage1_b'], X.coverage(1)[1])
        assert list(fz['contrast_weights']) == wts
    mc = json.load(open(js))['predictive']['contrast']
    assert mc['plan_b']['lags'] == [0, 2, 3] and [(s['drow'], s['dcol']) for s in mc['plan_b']['sites']] == [s[:2] for s in plan_b]
    assert mc['thresholds'] == THR and mc['labels'] == OUT and mc['members'] == 6 and mc['total_weight'] == 9
    assert mc['cell_area'] == X.cell_area and mc['levels'] == [0.5]
    assert mc['coverage_difference'] == [X.coverage_difference(k, (0.5,)) for k in range(2)]
    assert 'contrast' not in json.load(open(str(tmp_path / 'p' / 'pp.json')))['predictive']
    # a model of the union that fails for one member leaves that member out of every accumulator: lag 3 is
    # plan B's alone, so plan A's maps and the day-based ones skip the member too
    seen = []

    def failing(pop_model, lags, wind_data=None):
        made = real(pop_model, lags, wind_data)
        inner = made[3].evaluate

        def evaluate(*a, **k):
            seen.append(1)
            if len(seen) == 2:
                raise ValueError('no kernel for this member')
            return inner(*a, **k)
        made[3].evaluate = evaluate
        return made
    monkeypatch.setattr(PR, 'lagged_models', failing)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        pe = _pop_model(R, mode='exact')
        part = PR.posterior_predictive(pe, chains[:1], sites=arg, compare=cmp_arg, **kw)
    monkeypatch.setattr(PR, 'lagged_models', real)
    assert part.failed == 1 and part.evaluations == 3 and [r[1:] for r in part.runs] == [(0, 2), (3, 2)]
    for acc in (part.summary, part.arrival, part.sites.summary, part.sites.arrival, part.contrast):
        assert acc.members == 2 and acc.total_weight == 4
    assert list(part.contrast.weights) == [2, 2]
    _check_exact(part.contrast, _replay([fa[0], fa[2]], [fb[0], fb[2]], [2, 2], THR), 5)
    for k in range(2):
        for got, want in zip(part.contrast.coverage(k)[:2], X.coverage(k)[:2]):
            assert np.array_equal(got, want[[0, 2]])
    for r in (res, par, plain, part):
        for acc in (r.summary, r.arrival, r.sites, r.contrast):
            if acc is not None:
                acc.close()
    for p in (pm, pa, pb, pc, pd, pe) + tuple(late.values()):
        p.close()


def test_refusals_at_the_c_abi_and_the_handle_stays_usable():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import PlanContrast, Projection, ReleaseSites, exposure_weights, lagged_models
    lib = L.load()
    dev = L.default_device()
    h = L._VP()

    def create(thr, N=129, nslot=3, device=dev):
        t = L.f64(thr if len(thr) else [0.0])
        return lib.ps_contrast_create(device, N, nslot, len(thr), L.p_f64(t), C.byref(h))
    assert create([1, 2, 3, 4, 5]) == L.PS_ERR_BAD_ARG and not h
    for bad in ([0.0], [-1.0], [np.nan], [np.inf], [1.0, 1.0], [2.0, 1.0]):
        assert create(bad) == L.PS_ERR_BAD_ARG and not h
    assert b'threshold' in lib.ps_last_error()
    assert create([1.0], nslot=0) == L.PS_ERR_BAD_ARG and not h
    assert create([1.0], device=99) == L.PS_ERR_NO_DEVICE and not h
    assert create([1.0, 2.0, 3.0, 4.0], N=60001, nslot=32) == L.PS_ERR_OOM and not h      # 5.5 TB
    assert b'GB free' in lib.ps_last_error()
    assert create([]) == L.PS_OK and h
    lib.ps_contrast_destroy(h)
    pm, big = _pop_model(R), _pop_model(128)
    late = lagged_models(pm, [2])
    cells = [(0, 0, 1.0, 0), (3, 5, 0.5, 0)]
    out = np.empty((N, N))
    cnt = np.empty((N, N), dtype=np.uint32)
    u32 = C.POINTER(C.c_uint32)
    with ReleaseSites(pm, _metres(cells, R), [0, 2, 5]) as A, ReleaseSites(pm, _metres(cells[:1], R), [0, 2, 5]) as B, \
            ReleaseSites(big, _metres(cells, 128), [0, 2, 5]) as B128, ReleaseSites(pm, _metres(cells, R), [0, 2]) as B2, \
            ReleaseSites(pm, _metres(STAGGERED, R), [0, 2, 5], late) as Bst, \
            Projection(pm, exposure_weights(DAYS, [0, 2, 5]), DAYS) as PA, PlanContrast(A, B, THR) as X:
        X.profile(True)
        # before the first add, and before the plans hold anything
        assert lib.ps_contrast_fetch(X._h, 0, 0, L.p_f64(out)) == L.PS_ERR_STATE
        assert lib.ps_contrast_fetch_counts(X._h, 0, 0, cnt.ctypes.data_as(u32)) == L.PS_ERR_STATE
        assert lib.ps_contrast_add_sites(X._h, A._h, B._h, 1) == L.PS_ERR_STATE
        for m in (pm, big):
            _evaluate(m, MEMBERS[0])
        _evaluate(late[2], MEMBERS[0], ndays=4)
        for plan in (A, B128, B2):
            plan.apply()
        assert lib.ps_contrast_add_sites(X._h, A._h, B._h, 1) == L.PS_ERR_STATE            # B not applied yet
        B.apply()
        L.check(lib.ps_sites_apply(Bst._h, *Bst._calls()[0]))
        assert lib.ps_contrast_add_sites(X._h, A._h, Bst._h, 1) == L.PS_ERR_STATE          # B mid-pass over its groups
        assert b'group 1 of 2' in lib.ps_last_error()
        assert lib.ps_contrast_add_sites(X._h, Bst._h, A._h, 1) == L.PS_ERR_STATE
        for a, b, w, msg in ((A._h, A._h, 1, b'same release plan'), (A._h, B128._h, 1, b'domain 257'),
                             (B128._h, A._h, 1, b'domain 257'), (A._h, B2._h, 1, b'has 2 outputs'),
                             (A._h, B._h, 0, b'weight must be >= 1'), (A._h, None, 1, b'bad arguments'),
                             (None, B._h, 1, b'bad arguments')):
            assert lib.ps_contrast_add_sites(X._h, a, b, w) == L.PS_ERR_BAD_ARG
            assert msg in lib.ps_last_error(), (msg, lib.ps_last_error())
        assert lib.ps_contrast_add_sites(None, A._h, B._h, 1) == L.PS_ERR_BAD_ARG
        assert lib.ps_contrast_add_project(X._h, PA._h, PA._h, 1) == L.PS_ERR_BAD_ARG      # the same projection twice
        assert X.members == 0 and X.total_weight == 0 and X.profile()[1] == 0             # nothing was enqueued
        X.add(2)
        assert lib.ps_contrast_add_sites(X._h, A._h, B._h, 0xfffffffe) == L.PS_ERR_BAD_ARG  # W past 2^32 - 1
        assert b'overflow' in lib.ps_last_error()
        for slot, what in ((-1, 0), (3, 0), (0, -1), (0, 8)):
            assert lib.ps_contrast_fetch(X._h, slot, what, L.p_f64(out)) == L.PS_ERR_BAD_ARG
        for slot, which in ((3, 0), (0, -1), (0, 6)):
            assert lib.ps_contrast_fetch_counts(X._h, slot, which, cnt.ctypes.data_as(u32)) == L.PS_ERR_BAD_ARG
        assert lib.ps_contrast_fetch_coverage(X._h, 0, 2, None, None) == L.PS_ERR_BAD_ARG
        assert lib.ps_contrast_fetch_coverage(X._h, -1, 1, None, None) == L.PS_ERR_BAD_ARG
        with PlanContrast(A, B, [1.0]) as other:
            assert lib.ps_contrast_merge(X._h, other._h) == L.PS_ERR_BAD_ARG               # other thresholds
        assert lib.ps_contrast_merge(X._h, X._h) == L.PS_ERR_BAD_ARG
        assert X.members == 1 and X.total_weight == 2 and X.profile()[1] == 1
        # the handle still works: one member of weight 2
        fa, fb = [[A.field(e) for e in range(3)]], [[B.field(e) for e in range(3)]]
        _check_exact(X, _replay(fa, fb, [2], THR), 3)
        assert not X.variance(1).any() and X.counts(2, 0).max() == 2 and not X.counts(2, 1).any()
    for m in (pm, big, late[2]):
        m.close()


def test_the_grid_stride_path():
    """at R = 64 every launch is a single pass; the cell counts carried in a register over the grid stride only
    show once the pairs of cells exceed the launch cap of 4096 x 256, from R = 724 on: R = 768, 2 days, 2 members,
    single-group plans, plan B with a site on the south-east corner so that the tail cell counts too"""
    from parasitoids_amd.predictive import PlanContrast, ReleaseSites
    big = 768
    n = 2 * big + 1
    assert (n * n) // 2 > 4096 * 256 and (n * n) % 2 == 1
    pm = _pop_model(big, ndays=2)
    plan_a = [(0, 0, 1.0, 0), (700, -25, 0.5, 0)]                    # the second site beyond the grid's first pass
    plan_b = [(0, 0, 0.7, 0), (-30, 60, 0.8, 0), (big, big, 0.5, 0)]
    thr = [1.0, 100.0]
    fa, fb = [], []
    with ReleaseSites(pm, _metres(plan_a, big), [0, 1]) as A, ReleaseSites(pm, _metres(plan_b, big), [0, 1]) as B, \
            PlanContrast(A, B, thr) as X:
        assert [(s['drow'], s['dcol']) for s in B.sites] == [c[:2] for c in plan_b]
        for mem, w in zip(MEMBERS[:2], WEIGHTS[:2]):
            _evaluate(pm, mem)
            A.apply()
            B.apply()
            X.add(w)
            fa.append([A.field(e) for e in range(2)])
            fb.append([B.field(e) for e in range(2)])
        ref = _replay(fa, fb, WEIGHTS[:2], thr)
        assert fb[0][0][n - 1, n - 1] >= thr[1] and ref[0]['neg'][n - 1, n - 1] == 4 and ref[0]['loss'][1][n - 1, n - 1] == 4
        # cells beyond the first pass of the grid (flat index >= 2 x 4096 x 256) on both sides of the counts
        first_pass = 2 * 4096 * 256
        assert (fa[0][1].ravel()[first_pass:] >= thr[0]).sum() > 0 and (fb[0][1].ravel()[first_pass:] >= thr[0]).sum() > 0
        assert ref[1]['pos'].ravel()[first_pass:].max() > 0
        _check_exact(X, ref, 2)
    pm.close()
