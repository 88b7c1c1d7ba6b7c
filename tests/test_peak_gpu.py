"""GPU tests of the posterior peak maps (ps_peak_*, predictive.PeakMaps): the peak field, the peak-day and duration
counts, probabilities, quantiles and mean durations against the numpy reference built from
`PopModel.population(d)`, the ties to ArrivalMaps and SpreadSummary filled in the same run, day subsets, one
slot, 18 slots, no thresholds, weights, add and merge order, solver switches, reset, release plans and
projections as sources, the refusals, and posterior_predictive with peak thresholds.  Kalbar wind, R = 128,
6 days (N = 257: N * N is odd, so the pair path and the tail cell both run), the members, weights and helpers
of test_arrival_gpu.py."""
import ctypes as C
import json
import warnings

import numpy as np
import pytest

import peak_ref as R
import test_arrival_gpu as TA

pytestmark = pytest.mark.gpu

MEMBERS, WEIGHTS, THR, THR4, LEVELS = TA.MEMBERS, TA.WEIGHTS, TA.THR, TA.THR4, TA.LEVELS
_pop_model, _evaluate, _fields = TA._pop_model, TA._evaluate, TA._fields


def _check_against_reference(P, fields, weights, thr):
    """every device map of P against the numpy reference of the members' [nslot, N, N] fields -> (dc, uc)"""
    days, ns = P.days, len(P.days)
    dc = R.day_counts(fields, weights)
    prob = R.day_prob(dc)
    for s, d in enumerate(days):
        got = P.day_counts(d)
        assert got.dtype == np.uint32 and got.shape == dc.shape[1:]
        assert np.array_equal(got.astype(np.int64), dc[s]), d
        assert np.array_equal(P.day_prob(d), prob[s]), d
    for p in LEVELS:
        q = R.day_quantile(dc, p)
        got = P.day_quantile(p)
        assert got.dtype == np.int32 and np.array_equal(got, np.where(q < 0, -1, np.asarray(days)[q.clip(0)])), p
    uc = R.duration_counts(fields, weights, thr)
    for k in range(len(thr)):
        dprob = R.duration_prob(uc[k])
        for n in range(ns + 1):
            got = P.duration_counts(k, n)
            assert got.dtype == np.uint32 and np.array_equal(got.astype(np.int64), uc[k, n]), (k, n)
            if n:
                assert np.array_equal(P.duration_prob(k, n), dprob[n]), (k, n)
        for p in LEVELS:
            got = P.duration_quantile(k, p)
            assert got.dtype == np.int32 and np.array_equal(got, R.duration_quantile(uc[k], p)), (k, p)
        assert np.array_equal(P.duration_mean(k), R.duration_mean(uc[k])), k
    assert P.total_weight == sum(weights) and P.members == len(weights)
    return dc, uc


def _all_maps(P):
    """every integer and floating-point map of P, for bit-for-bit comparisons between handles"""
    out = [P.day_counts(d) for d in P.days] + [P.day_prob(d) for d in P.days]
    out += [P.day_quantile(p) for p in (0.05, 0.5, 1.0)]
    for k in range(len(P.thresholds)):
        out += [P.duration_counts(k, n) for n in range(len(P.days) + 1)]
        out += [P.duration_prob(k, n) for n in range(1, len(P.days) + 1)]
        out += [P.duration_quantile(k, p) for p in (0.05, 0.5, 1.0)] + [P.duration_mean(k)]
    return out


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


def _welford_mean(values, weights):
    """the statements of the summary's add kernel (weighted Welford, West 1979) on the members' fields"""
    m = np.zeros_like(values[0])
    W = 0.0
    for v, w in zip(values, weights):
        W = W + float(w)
        d = v - m
        m = m + d * float(w) / W
    return m


@pytest.mark.parametrize('prob_model', [False, True])
@pytest.mark.parametrize('mode', ['exact', None])
def test_device_maps_match_the_numpy_reference(prob_model, mode):
    from parasitoids_amd.predictive import ArrivalMaps, PeakMaps, SpreadSummary
    pm = _pop_model(prob_model=prob_model, **({} if mode is None else {'mode': mode}))
    days = list(range(6))
    scale = 1.0 / 130000 if prob_model else 1.0     # prob_model holds probabilities: the same densities
    thr, thr4 = [t * scale for t in THR], [t * scale for t in THR4]
    fields = []
    with PeakMaps(pm, thr) as P, PeakMaps(pm, thr4, days) as P4, ArrivalMaps(pm, thr) as A, \
            SpreadSummary(pm, days, thr) as S, SpreadSummary.for_projection(P, thr) as SP:
        assert P.days == days and P.N == 257 and P.consecutive and P.thresholds == thr
        for mem, w in zip(MEMBERS, WEIGHTS):
            _evaluate(pm, mem)
            for acc in (P, P4, A, S, SP):             # SP after P: it takes the peak field P has just written
                acc.add(w)
            fields.append(_fields(pm, days))
            m = R.peak_field(fields[-1])
            assert np.array_equal(P.field(), m) and np.array_equal(P4.field(), m)
        dc, uc = _check_against_reference(P, fields, WEIGHTS, thr)
        _check_against_reference(P4, fields, WEIGHTS, thr4)
        # not vacuous: peaks before the last day and on it, durations strictly inside 0..nslot, fewer of them higher up
        assert dc[:5].sum() > 0 and dc[5].sum() > 0
        inside = [int((uc[k, 1:6].sum(0) > 0).sum()) for k in range(2)]
        assert inside[0] > 0 and 0 < inside[1] < inside[0]
        W = sum(WEIGHTS)
        for k in range(2):
            # peak >= t is the same event as reaching t by the last day
            assert np.array_equal(SP.exceedance(0, k), A.prob_by(k, days[-1])), k
            ever = sum(P.duration_counts(k, n).astype(np.int64) for n in range(1, 7))
            never = A.counts(k, None)
            assert np.array_equal(ever, W - never.astype(np.int64)) and np.array_equal(P.duration_counts(k, 0), never)
            # at most 32 correctly rounded count / W <= 1 summed, against one rounded quotient <= 32: fewer than
            # 40 roundings of 1.1e-16 relative on values <= 32, about 1.4e-13
            total = sum(S.exceedance(d, k) for d in days)
            assert np.abs(P.duration_mean(k) - total).max() <= 1e-12, k
        assert np.array_equal(SP.mean(0), _welford_mean([R.peak_field(f) for f in fields], WEIGHTS))
        assert SP.members == len(MEMBERS) and SP.total_weight == W
    pm.close()


def test_a_day_subset_counts_listed_days_only():
    from parasitoids_amd.predictive import PeakMaps
    pm = _pop_model()
    sub = [1, 3, 4]
    fields = []
    with PeakMaps(pm, THR, sub) as P, PeakMaps(pm, THR, [3]) as P1, PeakMaps(pm) as P0:
        assert not P.consecutive and P1.consecutive and P0.consecutive and P0.thresholds == []
        for mem, w in zip(MEMBERS, WEIGHTS):
            _evaluate(pm, mem)
            for acc in (P, P1, P0):
                acc.add(w)
            fields.append(_fields(pm, list(range(6))))
            assert np.array_equal(P0.field(), R.peak_field(fields[-1]))
        _check_against_reference(P, [f[sub] for f in fields], WEIGHTS, THR)
        # one slot: the peak day is that day wherever the field is positive, the duration 0 or 1
        dc, uc = _check_against_reference(P1, [f[[3]] for f in fields], WEIGHTS, THR)
        positive = sum(w * (f[3] > 0) for f, w in zip(fields, WEIGHTS))
        assert np.array_equal(P1.day_counts(3).astype(np.int64), positive) and positive.max() == sum(WEIGHTS)
        assert uc.shape[1] == 2 and np.all(P1.duration_quantile(0, 1.0) <= 1)
        # no thresholds: peak value and peak day only
        _check_against_reference(P0, fields, WEIGHTS, [])
        with pytest.raises(ValueError):
            P0.duration_counts(0, 0)
        with pytest.raises(ValueError):
            P.day_prob(2)
    pm.close()


def test_all_eighteen_days_at_r64():
    """more slots than the one record in flight, and than any other test here"""
    from parasitoids_amd.predictive import PeakMaps
    pm = _pop_model(R=64, ndays=18)
    fields = []
    with PeakMaps(pm, THR) as P:
        assert len(P.days) == 18 and P.N == 129
        for mem, w in zip(MEMBERS[:3], WEIGHTS[:3]):
            _evaluate(pm, mem)
            P.add(w)
            fields.append(_fields(pm, P.days))
            assert np.array_equal(P.field(), R.peak_field(fields[-1]))
        dc, uc = _check_against_reference(P, fields, WEIGHTS[:3], THR)
        assert (dc[:-1].sum((1, 2)) > 0).sum() >= 3 and uc[0, 7:].sum() > 0     # peaks spread over the days, long stays
    pm.close()


def test_weights_orders_merges_solver_switches_and_reset_change_no_bit():
    from parasitoids_amd.predictive import PeakMaps
    pm, pm2 = _pop_model(), _pop_model()
    hs = [PeakMaps(pm, THR) for _ in range(7)]
    fwd, rev, unit, a1, b1, a2, b2 = hs
    alt = PeakMaps(pm2, THR)                 # fed from two models in turn: a solver switch per member
    order = list(range(len(MEMBERS)))
    for i in order:
        src = pm if i % 2 == 0 else pm2
        _evaluate(pm, MEMBERS[i])
        if src is pm2:
            _evaluate(pm2, MEMBERS[i])
        fwd.add(WEIGHTS[i])
        for _ in range(WEIGHTS[i]):
            unit.add(1)
        (a1 if i < 2 else b1).add(WEIGHTS[i])
        (a2 if i < 2 else b2).add(WEIGHTS[i])
        alt.pm = src
        alt.add(WEIGHTS[i])
    for i in reversed(order):
        _evaluate(pm, MEMBERS[i])
        rev.add(WEIGHTS[i])
    a1.merge(b1)              # first half + second half
    b2.merge(a2)              # second half + first half
    want = _all_maps(fwd)
    assert unit.members == sum(WEIGHTS) and unit.total_weight == fwd.total_weight == sum(WEIGHTS)
    for other in (rev, unit, a1, b2, alt):
        assert _same(_all_maps(other), want)
    last = fwd.field()
    fwd.reset()
    assert fwd.members == 0 and fwd.total_weight == 0
    for i in order:
        _evaluate(pm, MEMBERS[i])
        fwd.add(WEIGHTS[i])
    assert _same(_all_maps(fwd), want) and np.array_equal(fwd.field(), last)
    with PeakMaps(pm, THR) as e:             # merging into an empty handle
        e.merge(fwd)
        assert _same(_all_maps(e), want)
    for h in hs + [alt]:
        h.close()
    pm.close()
    pm2.close()


def test_release_plans_and_projections_as_sources():
    from parasitoids_amd.predictive import (PeakMaps, Projection, ReleaseSites, SpreadHistogram, SpreadSummary,
                                            exposure_weights, lagged_models)
    Rr = 64
    res = 10000.0 / Rr
    pm = _pop_model(R=Rr)
    out = [0, 1, 2, 3, 5]
    sites = [(0.0, 0.0, 0.6, 0), (13 * res, 6 * res, 0.5, 2)]          # the second site two days later
    late = lagged_models(pm, [2])
    W = exposure_weights(list(range(6)), [0, 2, 5])
    thr = [50.0, 500.0]
    plan_f, expo_f, day_f = [], [], []
    with ReleaseSites(pm, sites, out, late) as S, Projection(pm, W, list(range(6))) as X, \
            PeakMaps.for_projection(S, THR) as PS, PeakMaps.for_projection(X, thr) as PX, \
            PeakMaps(pm, THR) as PD, PeakMaps(pm, THR) as alone, \
            SpreadSummary.for_projection(PS, THR) as SS, SpreadHistogram.for_projection(PS) as HS:
        assert PS.days == out and not PS.consecutive and PX.days == [0, 1, 2] and PX.consecutive
        for mem, w in zip(MEMBERS[:3], WEIGHTS[:3]):
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)
                S.evaluate(TA.HP, mem[0], TA.DLP, mem[1], TA.NPER)       # the base model, the lagged one and the apply
            X.apply()
            for acc in (PS, SS, HS, PX, PD):
                acc.add(w)
            plan_f.append(np.array([S.field(e) for e in range(len(out))]))
            expo_f.append(np.array([X.field(e) for e in range(3)]))
            day_f.append(_fields(pm, PD.days))
            assert np.array_equal(PS.field(), R.peak_field(plan_f[-1]))
            assert np.array_equal(PX.field(), R.peak_field(expo_f[-1]))
        for mem, w in zip(MEMBERS[:3], WEIGHTS[:3]):       # the same members into a day-based handle on its own
            _evaluate(pm, mem)
            alone.add(w)
        dc, uc = _check_against_reference(PS, plan_f, WEIGHTS[:3], THR)
        assert dc[:-1].sum() > 0 and uc[0, 1:].sum() > 0
        dcx, _ = _check_against_reference(PX, expo_f, WEIGHTS[:3], thr)
        assert dcx[2].sum() > 0                                  # a cumulative sum that still grows peaks last
        _check_against_reference(PD, day_f, WEIGHTS[:3], THR)
        assert _same(_all_maps(PD), _all_maps(alone))
        assert np.array_equal(SS.mean(0), _welford_mean([R.peak_field(f) for f in plan_f], WEIGHTS[:3]))
        assert HS.members == 3 and HS.total_weight == sum(WEIGHTS[:3])
    for m in late.values():
        m.close()
    pm.close()


def test_refusals_enqueue_nothing_and_the_device_stays_usable():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import NEGVAL, PeakMaps, SpreadHistogram, SpreadSummary, _day_scales, _day_slots
    lib = L.load()
    dev = L.default_device()
    h = L._VP()
    thr5 = L.f64([1.0, 2.0, 3.0, 4.0, 5.0])
    assert lib.ps_peak_create(dev, 257, 33, 2, L.p_f64(thr5), C.byref(h)) == L.PS_ERR_BAD_ARG and not h
    assert lib.ps_peak_create(dev, 257, 6, 5, L.p_f64(thr5), C.byref(h)) == L.PS_ERR_BAD_ARG and not h
    assert lib.ps_peak_create(dev, 257, 6, 2, L.p_f64(L.f64([2.0, 1.0])), C.byref(h)) == L.PS_ERR_BAD_ARG and not h
    assert lib.ps_peak_create(dev, 257, 6, 2, L.p_f64(L.f64([0.0, 1.0])), C.byref(h)) == L.PS_ERR_BAD_ARG and not h
    assert lib.ps_peak_create(dev, 257, 6, 1, L.p_f64(L.f64([-1.0])), C.byref(h)) == L.PS_ERR_BAD_ARG and not h
    rc = lib.ps_peak_create(dev, 40001, 32, 4, L.p_f64(thr5), C.byref(h))       # ~1 TB
    assert rc == L.PS_ERR_OOM and not h and b'GB free' in lib.ps_last_error()
    pm = _pop_model()
    _evaluate(pm, MEMBERS[0])
    days = [1, 4]
    kind, idx, delta = _day_slots(days)
    stat, post = _day_scales(pm, days)

    def add(P, n, w, k=None):
        return lib.ps_peak_add(P._h, pm.solver._h, n, L.p_i32(kind if k is None else k), L.p_i32(idx), L.p_f64(stat),
                               L.p_f64(post), L.p_i32(delta), NEGVAL, w)
    with PeakMaps(pm, THR, days) as P, PeakMaps(pm, [1.0, 20.0], days) as other, \
            SpreadSummary.for_projection(P, THR) as S, SpreadHistogram.for_projection(P) as H:
        with pytest.raises(L.HipError) as err:
            P.day_quantile(0.5)                      # nothing accumulated
        assert err.value.code == L.PS_ERR_STATE
        with pytest.raises(L.HipError) as err:
            P.field()
        assert err.value.code == L.PS_ERR_STATE
        assert lib.ps_summary_add_peak(S._h, P._h, 1) == L.PS_ERR_STATE       # no peak field yet
        assert lib.ps_hist_add_peak(H._h, P._h, 1) == L.PS_ERR_STATE
        assert add(P, 3, 1) == L.PS_ERR_BAD_ARG                               # wrong slot count
        assert add(P, 2, 0) == L.PS_ERR_BAD_ARG                               # weight 0
        assert add(P, 2, 1, L.i32([L.REC_CHAIN, 99])) != L.PS_OK              # a bad slot: nothing enqueued
        assert P.members == 0 and P.total_weight == 0 and S.members == 0 and H.members == 0
        P.add(0xfffffffe)
        assert add(P, 2, 2) == L.PS_ERR_BAD_ARG and b'overflow' in lib.ps_last_error()   # W past 2^32 - 1
        assert P.members == 1 and P.total_weight == 0xfffffffe
        P.add(1)
        X = _fields(pm, days)
        assert np.array_equal(P.day_counts(4).astype(np.int64), 0xffffffff * (R.peak_slot(X) == 1))
        P.reset()
        other.add(1)
        with pytest.raises(L.HipError) as err:
            P.merge(other)                           # different thresholds
        assert err.value.code == L.PS_ERR_BAD_ARG
        with pytest.raises(L.HipError) as err:
            P.field()                                # and no peak field after a reset
        assert err.value.code == L.PS_ERR_STATE
        P.add(2)
        S.add(2)
        H.add(2)
        _check_against_reference(P, [X], [2], THR)
        assert np.array_equal(S.mean(0), R.peak_field(X)) and H.members == 1
    pm.close()


def _chain(run_lengths):
    """a short synthetic chain: runs of identical model parameters around the sampler's start values"""
    from parasitoids_amd import mcmc
    names = [m[0] for m in mcmc.MODEL_BLOCK]
    base = np.array([m[2] for m in mcmc.MODEL_BLOCK], dtype=np.float64)
    rows = []
    for n, length in enumerate(run_lengths):
        t = base.copy()
        t[names.index('sig_x')] += 6.0 * n
        t[names.index('sig_y')] -= 4.0 * n
        t[names.index('mu_r')] += 0.03 * n
        rows += [t] * length
    return np.array(rows), names


def _csr(f, key, N):
    from scipy import sparse
    return sparse.csr_matrix((f[key + '_data'], f[key + '_ind'], f[key + '_indptr']), shape=(N, N)).toarray()


def test_posterior_predictive_with_peak_maps(tmp_path):
    from parasitoids_amd import mcmc
    from parasitoids_amd import predictive as PR
    Rr, N = 64, 129
    trace, names = _chain([2, 1, 3, 1, 2])
    chains = [(trace[:5], names), (trace[5:], names)]       # the run of three is cut in two: 2 + 1 + 2 | 1 + 1 + 2
    kw = dict(thresholds=[1, 10], arrival=[1, 10], quantiles=[0.5])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        one, pa, pb = (_pop_model(R=Rr, mode='exact') for _ in range(3))
        res = PR.posterior_predictive(one, chains, peak=[1, 10], **kw)
        two = PR.posterior_predictive([pa, pb], chains, peak=dict(thresholds=[1, 10], levels=(0.5,)), **kw)
        plain = PR.posterior_predictive(one, chains, **kw)
    assert plain.peak is None and res.failed == 0 and res.evaluations == 6 and len(res.runs) == 6
    pk = res.peak
    assert pk.levels == [0.05, 0.5, 0.95] and two.peak.levels == [0.5]
    assert pk.maps.days == list(range(6)) and pk.maps.thresholds == [1.0, 10.0] and pk.summary.thresholds == [1.0, 10.0]
    for acc in (pk.maps, pk.summary, pk.histogram):
        assert acc.total_weight == res.summary.total_weight == 9 and acc.members == res.summary.members == 6
    # by hand: every run once more through the class, and through the numpy reference
    cols = [names.index(m[0]) for m in mcmc.MODEL_BLOCK]
    fields, weights = [], []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        with PR.PeakMaps(pa, [1, 10]) as P:
            for ci, first, weight in res.runs:
                pa.evaluate(*mcmc.model_args(chains[ci][0][first, cols]), want_stats=False)
                P.add(weight)
                fields.append(_fields(pa, P.days))
                weights.append(weight)
            hand = _all_maps(P)
    assert weights == [2, 1, 2, 1, 1, 2]
    _check_against_reference(pk.maps, fields, weights, [1.0, 10.0])
    assert _same(_all_maps(pk.maps), hand) and _same(_all_maps(two.peak.maps), hand)     # two models, merged
    # two chains: the merged mean is ps_summary_merge's pooled one, a few roundings from the sequential loop
    mean = _welford_mean([R.peak_field(f) for f in fields], weights)
    np.testing.assert_allclose(pk.summary.mean(0), mean, rtol=1e-12, atol=1e-12 * mean.max())
    for k in range(2):
        assert np.array_equal(pk.summary.exceedance(0, k), res.arrival.prob_by(k, 5))
        assert np.array_equal(two.peak.summary.exceedance(0, k), pk.summary.exceedance(0, k))
    assert np.array_equal(two.peak.histogram.counts(0), pk.histogram.counts(0))
    npz, js = res.save(str(tmp_path / 'a' / 'pp'))
    npz_p, js_p = plain.save(str(tmp_path / 'p' / 'pp'))
    assert not (tmp_path / 'p' / 'pp_peak.npz').exists()
    with np.load(npz) as fa, np.load(npz_p) as fp:          # the main file does not know about the peak maps
        assert set(fa.files) == set(fp.files) and all(np.array_equal(fa[key], fp[key]) for key in fp.files)
    want = {'days', 'peak_thresholds', 'peak_days', 'peakday_counts', 'days0_counts', 'days1_counts'}
    want |= {'%s_%s' % (name, q) for name in ('peakday', 'days0', 'days1') for q in ('q5', 'q50', 'q95')}
    with np.load(str(tmp_path / 'a' / 'pp_peak.npz')) as fz:
        for key, m in (('peak', pk.summary.mean(0)), ('peak_sd', pk.summary.sd(0)),
                       ('peak_pexc0', pk.summary.exceedance(0, 0)), ('peak_pexc1', pk.summary.exceedance(0, 1)),
                       ('peak_q50', pk.histogram.quantile(0, 0.5)), ('days0_mean', pk.maps.duration_mean(0)),
                       ('days1_mean', pk.maps.duration_mean(1))):
            assert np.array_equal(_csr(fz, key, N), np.where(m >= 1e-8, m, 0.0)), key
            want |= {'%s_%s' % (key, t) for t in ('data', 'ind', 'indptr')}
        assert set(fz.files) == want
        assert fz['peak_thresholds'].tolist() == [1.0, 10.0] and fz['peak_days'].tolist() == list(range(6))
        assert [str(x) for x in fz['days']] == ['peak', 'days0', 'days1']
        assert fz['peakday_q50'].dtype == np.int16 and np.array_equal(fz['peakday_q50'], pk.maps.day_quantile(0.5))
        assert np.array_equal(fz['days1_q95'], pk.maps.duration_quantile(1, 0.95))
        assert fz['peakday_counts'].shape == (6, N, N) and fz['days0_counts'].shape == (7, N, N)
        assert np.array_equal(fz['peakday_counts'][2], pk.maps.day_counts(2))
        assert np.array_equal(fz['days0_counts'][0], pk.maps.duration_counts(0, 0))
        assert np.all(fz['days1_counts'].sum(0) == 9)
    meta = json.load(open(js))['predictive']['peak']
    assert meta['thresholds'] == [1.0, 10.0] and meta['days'] == list(range(6)) and meta['levels'] == [0.05, 0.5, 0.95]
    assert meta['consecutive'] is True and meta['members'] == 6 and meta['total_weight'] == 9
    assert meta['max_mean_duration'] == [float(pk.maps.duration_mean(k).max()) for k in range(2)]
    assert 'peak' not in json.load(open(js_p))['predictive']
    for r in (res, two, plain):
        for acc in (r.summary, r.histogram, r.arrival, r.peak):
            if acc is not None:
                acc.close()
    for p in (one, pa, pb):
        p.close()


def test_posterior_predictive_gives_the_release_plan_peak_maps_of_its_own(tmp_path):
    from parasitoids_amd import mcmc
    from parasitoids_amd import predictive as PR
    Rr = 64
    res_m = 10000.0 / Rr
    out = [0, 1, 2, 3, 5]
    trace, names = _chain([2, 1, 2])
    arg = dict(sites=[(0.0, 0.0, 0.6), (13 * res_m, 6 * res_m, 0.5, 2)], days=out)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        pm = _pop_model(R=Rr, mode='exact')
        res = PR.posterior_predictive(pm, [(trace, names)], thresholds=[1, 10], peak=[1, 10], sites=arg,
                                      exposure=[0, 2, 5])
    assert res.exposure is not None and res.exposure.peak is None        # the projections get none here
    sp = res.sites.peak
    assert sp.maps.days == out and not sp.maps.consecutive and sp.histogram is None
    assert sp.maps.members == 3 and sp.maps.total_weight == 5 == sp.summary.total_weight
    cols = [names.index(m[0]) for m in mcmc.MODEL_BLOCK]
    plan_f = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        with PR.ReleaseSites.with_lagged_models(pm, arg['sites'], out) as P:
            for ci, first, weight in res.runs:
                P.evaluate(*mcmc.model_args(trace[first, cols]))
                plan_f.append(np.array([P.field(e) for e in range(len(out))]))
    _check_against_reference(sp.maps, plan_f, [2, 1, 2], [1.0, 10.0])
    assert np.array_equal(sp.summary.mean(0), _welford_mean([R.peak_field(f) for f in plan_f], [2, 1, 2]))
    npz, js = res.save(str(tmp_path / 'pp'))
    assert (tmp_path / 'pp_peak.npz').exists()
    with np.load(str(tmp_path / 'pp_sites_peak.npz')) as fz:
        assert fz['peak_days'].tolist() == out and np.array_equal(fz['peakday_q50'], sp.maps.day_quantile(0.5))
    meta = json.load(open(js))['predictive']
    assert meta['sites']['peak']['consecutive'] is False and meta['sites']['peak']['days'] == out
    assert meta['peak']['consecutive'] is True
    for acc in (res.summary, res.peak, res.sites, res.exposure):
        acc.close()
    pm.close()


def test_profile_counts_every_launch_of_a_long_lived_handle():
    """the handle folds finished event pairs into running totals (at most 256 pairs pending): 300 profiled adds
    and reads in between lose no launch, and the counts are those of 300 unit adds"""
    from parasitoids_amd.predictive import PeakMaps
    pm = _pop_model(R=64, ndays=3)
    _evaluate(pm, MEMBERS[0])
    with PeakMaps(pm, THR) as P, PeakMaps(pm, THR) as Q:
        pitch = (P.N * P.N + 63) // 64 * 64
        assert P.nbytes == 3 * 3 * pitch * 4 + 2 * pitch * 8      # counts, the peak field and the map scratch
        P.profile(True)
        for _ in range(120):
            P.add(1)
        ms0, n0 = P.profile()[:2]
        assert n0 == 120 and ms0 > 0
        for _ in range(180):
            P.add(1)
        P.day_prob(2)
        ms, n, map_ms, maps = P.profile()
        assert n == 300 and ms > ms0 and maps == 1 and map_ms > 0
        assert P.profile(False)[1] == 300
        P.add(1)
        assert P.profile()[1] == 300 and P.total_weight == 301
        Q.add(301)
        assert _same(_all_maps(P), _all_maps(Q))
    pm.close()
