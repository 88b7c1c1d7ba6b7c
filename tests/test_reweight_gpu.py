"""GPU tests of the reweighted summaries (ps_wsum_*, predictive.ReweightedSummary): mean and exceedance sums bit for
bit against the numpy loop of reweight_ref on `PopModel.population(d)`, the variance within the rule of
test_predictive_gpu._check, the tie of an all-zero scenario to SpreadSummary, day subsets, shift invariance of the
log-weights, add and merge order, projections and release plans as sources, the refusals, and posterior_predictive
with reweight=.  Kalbar wind, R = 128, 6 days (N = 257: N * N is odd, the tail cell is on its own), the members
and weights of test_arrival_gpu.py."""
import json
import math
import os
import types
import warnings

import numpy as np
import pytest

import reweight_ref as RR
from helpers import HP, DLP, NPER
from test_arrival_gpu import MEMBERS, WEIGHTS, THR, _pop_model, _evaluate, _fields

pytestmark = pytest.mark.gpu

INF = math.inf
LAM = {'flat': [0.0, 0.0, 0.0, 0.0, 0.0],
       'swing': [0.0, -1.5, 2.25, 2.25, -800.0],       # one rescale upward, the maximum again, one underflow
       'late': [-INF, 0.5, -0.25, 3.0, 1.0]}           # starts at the second member, two rescales
NAMES = ['flat', 'swing', 'late']


def _lams(names, m, shift=0.0):
    return [LAM[n][m] + shift for n in names]


def _maps(R, names, keys):
    """every map of every scenario: {(name, key, what): array}"""
    out = {}
    for n in names:
        for d in keys:
            out[n, d, 'mean'] = R.mean(n, d)
            out[n, d, 'var'] = R.variance(n, d)
            for k in range(len(R.thresholds)):
                out[n, d, k] = R.exceedance(n, d, k)
    return out


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def _check_state(R, st, names, keys):
    """mean and exceedance bit for bit, variance by the rule of test_predictive_gpu._check (rtol 1e-12, atol
    1e-15 scale^2), the host side equal"""
    for j, n in enumerate(names):
        sc = st[j]
        assert (R.members(n), R.skipped(n)) == (sc['members'], sc['skipped']), n
        assert R.log_total_weight(n) == RR.log_total_weight(sc), n
        for i, d in enumerate(keys):
            assert np.array_equal(R.mean(n, d), sc['mean'][i]), (n, d)
            scale = np.abs(sc['mean'][i]).max()
            np.testing.assert_allclose(R.variance(n, d), RR.variance(sc)[i], rtol=1e-12, atol=1e-15 * scale ** 2)
            for k in range(len(R.thresholds)):
                assert np.array_equal(R.exceedance(n, d, k), RR.exceedance(sc, k)[i]), (n, d, k)


def _check_close(A, B, names, keys, rtol=1e-12):
    """two handles within the project's merge tolerance (test_predictive_gpu._check)"""
    for n in names:
        assert abs(A.log_total_weight(n) - B.log_total_weight(n)) <= 1e-14 * max(1.0, abs(B.log_total_weight(n)))
        for d in keys:
            m = B.mean(n, d)
            scale = np.abs(m).max()
            np.testing.assert_allclose(A.mean(n, d), m, rtol=rtol, atol=rtol * 1e-3 * scale)
            np.testing.assert_allclose(A.variance(n, d), B.variance(n, d), rtol=rtol, atol=rtol * 1e-3 * scale ** 2)
            for k in range(len(A.thresholds)):
                np.testing.assert_allclose(A.exceedance(n, d, k), B.exceedance(n, d, k), rtol=rtol, atol=rtol * 1e-3)


@pytest.mark.parametrize('prob_model', [False, True])
def test_three_scenarios_in_one_handle_match_the_numpy_loop(prob_model):
    from parasitoids_amd.predictive import ReweightedSummary, SpreadSummary
    pm = _pop_model(prob_model=prob_model)
    days = list(range(6))
    scale = 1.0 / 130000 if prob_model else 1.0
    thr = [t * scale for t in THR]
    st = RR.new_state((6, 257, 257), thr, 3)
    with ReweightedSummary(pm, NAMES, days, thr) as R, SpreadSummary(pm, days, thr) as S:
        assert R.N == 257 and R.scenarios == NAMES and R.nbytes == 3 * 4 * 8 * 6 * 66112
        assert R.log_total_weight('late') == -INF
        for m, (mem, w) in enumerate(zip(MEMBERS, WEIGHTS)):
            _evaluate(pm, mem)
            S.add(w)
            R.add(_lams(NAMES, m), w)
            RR.add(st, _fields(pm, days), _lams(NAMES, m), w)
        _check_state(R, st, NAMES, days)
        assert [R.members(n) for n in NAMES] == [5, 4, 4] and [R.skipped(n) for n in NAMES] == [0, 1, 1]
        assert R.ref == [0.0, 2.25, 3.0] and R.total_weight('flat') == sum(WEIGHTS)
        assert R.mean('swing', 5).max() > 0 and not np.array_equal(R.mean('swing', 5), R.mean('flat', 5))
        assert R.variance('late', 4).max() > 0 and R.exceedance('late', 4, 1).max() > 0
        # the tie: with all log-weights 0 the handle holds the bits of the plain summary
        for d in days:
            assert np.array_equal(R.mean('flat', d), S.mean(d)), d
            assert np.array_equal(R.variance('flat', d), S.variance(d)), d
            for k in range(len(thr)):
                assert np.array_equal(R.exceedance('flat', d, k), S.exceedance(d, k)), (d, k)
        if prob_model:
            assert any(pm.stats[d].delta != 0.0 for d in range(5))
        # a dict of log-weights by name, and reset
        R.reset()
        assert R.ref == [-INF] * 3 and R.members('flat') == 0
        R.add({'late': 0.0, 'flat': -1.0, 'swing': -INF}, 2)
        assert (R.members('swing'), R.skipped('swing'), R.ref) == (0, 1, [-1.0, -INF, 0.0])
        assert np.array_equal(R.mean('late', 3), R.mean('flat', 3)) and R.total_weight('flat') == 2.0
    pm.close()


def test_day_subsets_and_eighteen_slots():
    from parasitoids_amd.predictive import ReweightedSummary
    names = ['swing', 'late']
    pm = _pop_model()
    with ReweightedSummary(pm, names, [1, 3, 4], THR) as A, ReweightedSummary(pm, names, [3], [10.0]) as B:
        sa, sb = RR.new_state((3, 257, 257), THR, 2), RR.new_state((1, 257, 257), [10.0], 2)
        for m, (mem, w) in enumerate(zip(MEMBERS, WEIGHTS)):
            _evaluate(pm, mem)
            A.add(_lams(names, m), w)
            B.add(_lams(names, m), w)
            RR.add(sa, _fields(pm, [1, 3, 4]), _lams(names, m), w)
            RR.add(sb, _fields(pm, [3]), _lams(names, m), w)
        _check_state(A, sa, names, [1, 3, 4])
        _check_state(B, sb, names, [3])
        assert np.array_equal(A.mean('late', 3), B.mean('late', 3))
        for d in (0, 2, 5):
            with pytest.raises(ValueError, match='not in the reweighted summary'):
                A.mean('swing', d)
        with pytest.raises(ValueError, match='not one of'):
            A.mean('flat', 3)
        with pytest.raises(ValueError, match='threshold'):
            B.exceedance('late', 3, 1)
    pm.close()
    pm = _pop_model(R=64, ndays=18)
    days = list(range(18))
    with ReweightedSummary(pm, names, None, [1.0]) as C:
        assert C.days == days and C.N == 129
        sc = RR.new_state((18, 129, 129), [1.0], 2)
        for m, (mem, w) in enumerate(zip(MEMBERS, WEIGHTS)):
            _evaluate(pm, mem)
            C.add(_lams(names, m), w)
            RR.add(sc, _fields(pm, days), _lams(names, m), w)
        _check_state(C, sc, names, days)
        assert C.mean('swing', 17).max() > 0
    pm.close()


def test_a_common_shift_of_the_log_weights_changes_nothing():
    """256 is a power of two: lambda + 256 is off by at most 2^-45, every omega by at most 2^-44 relative, and the
    mean is a convex combination of the members' values"""
    from parasitoids_amd.predictive import ReweightedSummary
    pm = _pop_model()
    days = list(range(6))
    with ReweightedSummary(pm, ['swing', 'shifted'], days, THR) as R:
        for m, (mem, w) in enumerate(zip(MEMBERS, WEIGHTS)):
            _evaluate(pm, mem)
            R.add([LAM['swing'][m], LAM['swing'][m] + 256.0], w)
        assert R.ref == [2.25, 258.25] and R.skipped('shifted') == R.skipped('swing') == 1
        assert abs(R.log_total_weight('shifted') - 256.0 - R.log_total_weight('swing')) < 1e-12
        for d in days:
            m = R.mean('swing', d)
            np.testing.assert_allclose(R.mean('shifted', d), m, rtol=0, atol=1e-12 * np.abs(m).max())
            v = R.variance('swing', d)
            np.testing.assert_allclose(R.variance('shifted', d), v, rtol=0, atol=1e-12 * np.abs(v).max())
            for k in range(2):
                np.testing.assert_allclose(R.exceedance('shifted', d, k), R.exceedance('swing', d, k), rtol=0,
                                           atol=1e-12)
    pm.close()


def test_add_order_and_merge_order():
    from parasitoids_amd.predictive import ReweightedSummary
    pm = _pop_model()
    days = [0, 2, 5]
    hs = [ReweightedSummary(pm, NAMES, days, THR) for _ in range(7)]
    one, a1, b1, a2, b2, empty, rev = hs
    for m, (mem, w) in enumerate(zip(MEMBERS, WEIGHTS)):
        _evaluate(pm, mem)
        lam = _lams(NAMES, m)
        one.add(lam, w)
        for h in ((a1, a2) if m < 2 else (b1, b2)):
            h.add(lam, w)
    for m in reversed(range(len(MEMBERS))):
        _evaluate(pm, MEMBERS[m])
        rev.add(_lams(NAMES, m), WEIGHTS[m])
    assert a1.ref == [0.0, 0.0, 0.5] and b1.ref == [0.0, 2.25, 3.0]        # the two sides sit on different scales
    before = _maps(b1, NAMES, days)
    info = [(b1.members(n), b1.skipped(n), b1.log_total_weight(n)) for n in NAMES]
    empty.merge(b1)                                    # into an empty handle: a copy, bit for bit
    assert _same(_maps(empty, NAMES, days), before) and empty.ref == b1.ref
    assert [(empty.members(n), empty.skipped(n), empty.log_total_weight(n)) for n in NAMES] == info
    a1.merge(b1)
    assert _same(_maps(b1, NAMES, days), before)       # src is unchanged
    assert [(b1.members(n), b1.skipped(n), b1.log_total_weight(n)) for n in NAMES] == info
    b2.merge(a2)                                       # the other order
    for h in (a1, b2, rev):
        assert h.ref == one.ref
        _check_close(h, one, NAMES, days)
    for h in (a1, b2):
        assert [(h.members(n), h.skipped(n)) for n in NAMES] == [(one.members(n), one.skipped(n)) for n in NAMES]
    assert [rev.members(n) for n in NAMES] == [5, 5, 4]       # -800 comes first there: a member, rescaled away later
    with ReweightedSummary(pm, NAMES, [0, 2, 4], THR) as other:
        with pytest.raises(ValueError, match='different days'):
            one.merge(other)
    for h in hs:
        h.close()
    pm.close()


def test_a_release_plan_and_an_emergence_projection_as_sources():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import (PeakMaps, Projection, ReleaseSites, ReweightedSummary, SpreadSummary,
                                            emergence_plan, lagged_models)
    pm = _pop_model()
    res = 10000.0 / 128
    late = lagged_models(pm, [0, 2])
    plan = [(0.0, 0.0, 0.6, 0), (13 * res, 6 * res, 0.4, 2)]
    W, in_days, labels = emergence_plan(dict(collection_day=5, obs_days=[24, 27]), 6)
    names = ['swing', 'late', 'flat']
    with Projection(pm, W, in_days) as P, ReleaseSites(pm, plan, [0, 2, 3, 5], late) as RS, \
            ReweightedSummary.for_projection(P, names, THR) as RP, \
            ReweightedSummary.for_projection(RS, names, THR) as RSs, SpreadSummary.for_projection(RS, THR) as S, \
            PeakMaps(pm, [], [1, 3, 5]) as PK, ReweightedSummary.for_projection(PK, names, THR) as RK:
        lib = RP._lib
        one = L.f64([1.0, 1.0, 1.0])
        assert lib.ps_wsum_add_project(RP._h, P._h, 3, L.p_f64(one), L.p_f64(one)) == L.PS_ERR_STATE   # nothing applied
        assert lib.ps_wsum_add_sites(RSs._h, RS._h, 3, L.p_f64(one), L.p_f64(one)) == L.PS_ERR_STATE
        assert lib.ps_wsum_add_peak(RK._h, PK._h, 3, L.p_f64(one), L.p_f64(one)) == L.PS_ERR_STATE
        assert RP.members('flat') == 0 and RSs.members('flat') == 0 and RK.members('flat') == 0
        sp, ss = RR.new_state((2, 257, 257), THR, 3), RR.new_state((4, 257, 257), THR, 3)
        sk = RR.new_state((1, 257, 257), THR, 3)
        for m, (mem, w) in enumerate(zip(MEMBERS, WEIGHTS)):
            _evaluate(pm, mem)
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)
                late[2].evaluate(HP, mem[0], DLP, mem[1], NPER, ndays=4, want_stats=False)
            P.apply()
            RS.apply()
            PK.add(w)
            lam = _lams(names, m)
            RP.add(lam, w)
            RSs.add(lam, w)
            RK.add(lam, w)
            S.add(w)
            RR.add(sk, PK.field()[None], lam, w)
            RR.add(sp, np.array([P.field(k) for k in range(2)]), lam, w)
            RR.add(ss, np.array([RS.field(k) for k in range(4)]), lam, w)
        assert RP.days == [0, 1] and RSs.days == [0, 1, 2, 3]
        _check_state(RP, sp, names, [0, 1])
        _check_state(RSs, ss, names, [0, 1, 2, 3])
        assert RK.days == [0]                           # the peak over days 1, 3, 5: one field per member
        _check_state(RK, sk, names, [0])
        assert RK.mean('swing', 0).max() > 0
        assert RP.mean('late', 1).max() > 0 and RSs.exceedance('swing', 3, 0).max() > 0
        for e in range(4):
            assert np.array_equal(RSs.mean('flat', e), S.mean(e)) and np.array_equal(RSs.variance('flat', e), S.variance(e))
    for m in (pm, late[2]):
        m.close()


def test_refusals_change_nothing():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import ReweightedSummary
    pm = _pop_model()
    small = _pop_model(R=64)
    days = [0, 3, 5]
    for bad in (['a', 'b', 'c', 'd', 'e'], ['a', 'a'], [], 'ab'):
        with pytest.raises(ValueError, match='scenario'):
            ReweightedSummary(pm, bad, days, THR)
    for thr in ([10.0, 1.0], [1.0, 1.0], [0.0, 1.0], [1.0, INF], [1, 2, 3, 4, 5]):
        with pytest.raises(ValueError):
            ReweightedSummary(pm, NAMES, days, thr)
    with pytest.raises(ValueError, match='slots'):
        ReweightedSummary(types.SimpleNamespace(days=list(range(40)), rad_res=64, device=0), NAMES, None, THR)
    lib = L.load()
    h = L._VP()
    import ctypes as C
    thr = L.f64([10.0, 1.0])
    assert lib.ps_wsum_create(0, 257, 2, 3, 2, L.p_f64(thr), C.byref(h)) == L.PS_ERR_BAD_ARG       # not increasing
    thr = L.f64([1.0, 10.0])
    for nscen, nslot, nthr in ((0, 3, 2), (5, 3, 2), (2, 0, 2), (2, 33, 2), (2, 3, 5)):
        assert lib.ps_wsum_create(0, 257, nscen, nslot, nthr, L.p_f64(thr), C.byref(h)) == L.PS_ERR_BAD_ARG
    with ReweightedSummary(pm, NAMES, days, THR) as R:
        with pytest.raises(ValueError, match='last evaluation'):
            R.add([0.0, 0.0, 0.0])                       # nothing evaluated yet
        _evaluate(pm, MEMBERS[0])
        _evaluate(small, MEMBERS[0])
        R.add(_lams(NAMES, 0), 1)
        _evaluate(pm, MEMBERS[1])
        R.add([0.0, -1.5, -INF], 3)
        with pytest.raises(L.HipError) as err:
            R.mean('late', 3)                            # an empty scenario
        assert err.value.code == L.PS_ERR_STATE
        names = NAMES[:2]
        before = _maps(R, names, days)
        host = [(R.members(n), R.skipped(n), R.log_total_weight(n)) for n in NAMES], list(R.ref)
        for lam in ([0.0, math.nan, 0.0], [INF, 0.0, 0.0], [0.0, 0.0], [0.0] * 4, 'abc', {'flat': 0.0}):
            with pytest.raises(ValueError):
                R.add(lam)
        for w in (0, -1, math.nan, INF):
            with pytest.raises(ValueError, match='weight'):
                R.add([0.0, 0.0, 0.0], w)
        # the library's own checks: every argument before anything is enqueued
        kind, idx, delta = R._kind, R._idx, R._delta
        stat, post = L.f64([130000.0, 1.0, 1.0]), L.f64([1.0, 130000.0, 130000.0])

        def add(solver, nslot, nscen, r, om):
            return lib.ps_wsum_add(R._h, solver._h, nslot, L.p_i32(kind), L.p_i32(idx), L.p_f64(stat), L.p_f64(post),
                                   L.p_i32(delta), 1e-8, nscen, L.p_f64(L.f64(r)), L.p_f64(L.f64(om)))
        ok = [1.0, 1.0, 1.0]
        assert add(small.solver, 3, 3, ok, ok) == L.PS_ERR_BAD_ARG and b'domain' in lib.ps_last_error()
        assert add(pm.solver, 2, 3, ok, ok) == L.PS_ERR_BAD_ARG
        assert add(pm.solver, 3, 2, ok, ok) == L.PS_ERR_BAD_ARG
        assert add(pm.solver, 3, 4, ok + [1.0], ok + [1.0]) == L.PS_ERR_BAD_ARG
        for om in ([1.0, math.nan, 1.0], [1.0, 1.0, -0.5], [INF, 1.0, 1.0]):
            assert add(pm.solver, 3, 3, ok, om) == L.PS_ERR_BAD_ARG and b'omega' in lib.ps_last_error()
        for r in ([1.5, 1.0, 1.0], [1.0, -0.1, 1.0], [1.0, 1.0, math.nan]):
            assert add(pm.solver, 3, 3, r, ok) == L.PS_ERR_BAD_ARG and b'rescale' in lib.ps_last_error()
        bad_idx = L.i32([0, 2, 9])                       # chain record 9 of a 6-day run: the third descriptor
        assert lib.ps_wsum_add(R._h, pm.solver._h, 3, L.p_i32(kind), L.p_i32(bad_idx), L.p_f64(stat), L.p_f64(post),
                               L.p_i32(delta), 1e-8, 3, L.p_f64(L.f64(ok)), L.p_f64(L.f64(ok))) != L.PS_OK
        assert lib.ps_wsum_fetch(R._h, 3, 0, 0, L.p_f64(np.empty((257, 257)))) == L.PS_ERR_BAD_ARG
        assert lib.ps_wsum_fetch(R._h, 0, 3, 0, L.p_f64(np.empty((257, 257)))) == L.PS_ERR_BAD_ARG
        assert lib.ps_wsum_fetch(R._h, 0, 0, 4, L.p_f64(np.empty((257, 257)))) == L.PS_ERR_BAD_ARG
        assert lib.ps_wsum_merge(R._h, R._h, L.p_f64(L.f64(ok)), L.p_f64(L.f64(ok))) == L.PS_ERR_BAD_ARG
        with ReweightedSummary(small, NAMES, days, THR) as other:
            assert lib.ps_wsum_merge(R._h, other._h, L.p_f64(L.f64(ok)), L.p_f64(L.f64(ok))) == L.PS_ERR_BAD_ARG
        # after all of them every plane and the host side are bit for bit what they were
        assert _same(_maps(R, names, days), before)
        assert ([(R.members(n), R.skipped(n), R.log_total_weight(n)) for n in NAMES], list(R.ref)) == host
        with pytest.raises(L.HipError):
            R.mean('late', 3)
    pm.close()
    small.close()


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


def test_posterior_predictive_with_reweight_and_a_release_plan(tmp_path):
    from parasitoids_amd import mcmc
    from parasitoids_amd import predictive as PR
    N = 257
    res_m = 10000.0 / 128
    trace, names = _chain([3, 2, 4, 3])
    chain = (trace, names)
    given = [(0, 0, 1, 'count', 1e-3, 3), (3000, 0, 2, 'found', 0.5)]
    rw = {'trap': dict(probes=given), 'flat': dict(log_weights=[np.zeros(12)])}
    out = [0, 2, 3, 5]
    arg = dict(sites=[(0.0, 0.0, 0.6), (13 * res_m, 6 * res_m, 0.5, 2)], days=out)
    pm = _pop_model(mode='exact')       # an auto-mode model routes days by what it has seen: the runs are repeated below
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        with pytest.warns(UserWarning, match='effective sample size'):
            res = PR.posterior_predictive(pm, chain, thresholds=THR, reweight=rw, sites=arg)
    R, S = res.reweight, res.summary
    assert res.failed == 0 and res.evaluations == 4 and R.scenarios == ['trap', 'flat'] and R.days == S.days
    # flat: log-weights 0 on every row, so every run's log-weight is 0: the plain summary, bit for bit
    for d in S.days:
        assert np.array_equal(R.mean('flat', d), S.mean(d)) and np.array_equal(R.variance('flat', d), S.variance(d))
        for k in range(2):
            assert np.array_equal(R.exceedance('flat', d, k), S.exceedance(d, k))
    # trap: every run once more through the model by hand, the probes from the device's own gathered values
    cols = [names.index(m[0]) for m in mcmc.MODEL_BLOCK]
    st = RR.new_state((6, N, N), THR, 2)
    sp = RR.new_state((4, N, N), THR, 2)
    rows_l, zero = [], 0
    prow, pcol = [128, 128], [128, 128 + int(np.around(3000 / res_m))]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        with PR.ReleaseSites.with_lagged_models(pm, arg['sites'], out) as P:
            for ci, first, weight in res.runs:
                P.evaluate(*mcmc.model_args(trace[first, cols]))
                got = pm.gather_days([1, 2], prow, pcol)
                vals = [got[0, 0], got[1, 1]]
                assert vals[0] > 0                      # the release cell one day on: every member holds wasps there
                zero += int(vals[1] == 0.0)
                lam = RR.probes_loglik(given, vals)
                rows_l += [lam] * weight
                RR.add(st, _fields(pm, S.days), [lam, 0.0], weight)
                RR.add(sp, np.array([P.field(e) for e in range(len(out))]), [lam, 0.0], weight)
    _check_state(R, st, ['trap', 'flat'], S.days)
    assert R.skipped('trap') == zero == st[0]['skipped'] and R.members('trap') == 4 - zero >= 2
    rel = max(np.abs(R.mean('trap', d) - S.mean(d)).max() / np.abs(S.mean(d)).max() for d in S.days)
    assert rel > 1e-6                                   # the probes do move the maps
    # the diagnostics, from the rows' log-weights
    info = res.reweight_info
    assert info['names'] == ['trap', 'flat'] and info['probes'] == [[list(p) for p in given], None]
    want = RR.diagnostics(rows_l)
    got = info['diagnostics']['trap']
    assert {k: got[k] for k in want} == want and got['rows'] == 12
    assert (got['members'], got['skipped'], got['log_total_weight']) == (4 - zero, zero, RR.log_total_weight(st[0]))
    flat = info['diagnostics']['flat']
    assert (flat['rows'], flat['skipped_rows'], flat['ess'], flat['max_share'], flat['log_mean_weight']) == \
        (12, 0, 12.0, 1.0 / 12, 0.0)
    # the plan has its own maps
    RSs = res.sites.reweight
    assert RSs.days == [0, 1, 2, 3] and RSs.scenarios == ['trap', 'flat']
    _check_state(RSs, sp, ['trap', 'flat'], [0, 1, 2, 3])
    for e in range(4):
        assert np.array_equal(RSs.mean('flat', e), res.sites.summary.mean(e))
    # the files
    npz, js = res.save(str(tmp_path / 'a' / 'pp'))
    f = np.load(str(tmp_path / 'a' / 'pp_reweight.npz'))
    assert [str(n) for n in f['scenarios']] == ['trap', 'flat']
    labels = [pm.days[d] for d in S.days]
    assert [str(x) for x in f['labels']] == [str(x) for x in labels]
    for j, n in enumerate(['trap', 'flat']):
        for d, label in zip(S.days, labels):
            m = R.mean(n, d)
            assert np.array_equal(_csr(f, 's%d_%s' % (j, label), N), np.where(m >= 1e-8, m, 0.0))
            sd = R.sd(n, d)
            assert np.array_equal(_csr(f, 's%d_%s_sd' % (j, label), N), np.where(sd >= 1e-8, sd, 0.0))
            p = R.exceedance(n, d, 1)
            assert np.array_equal(_csr(f, 's%d_%s_pexc1' % (j, label), N), np.where(p >= 1e-8, p, 0.0))
    fs = np.load(str(tmp_path / 'a' / 'pp_sites_reweight.npz'))
    m = RSs.mean('trap', 3)
    assert np.array_equal(_csr(fs, 's0_%s' % out[3], N), np.where(m >= 1e-8, m, 0.0))
    meta = json.load(open(js))['predictive']['reweight']
    assert meta['names'] == ['trap', 'flat'] and meta['days'] == S.days and meta['thresholds'] == THR
    assert meta['probes'] == [[list(p) for p in given], None] and meta['min_ess'] == 50.0
    assert meta['diagnostics']['trap']['ess'] == got['ess'] and meta['diagnostics']['flat']['rows'] == 12
    # no warning where the caller lowers the bar; a scenario no member is compatible with is named
    with warnings.catch_warnings():
        warnings.simplefilter('error', UserWarning)
        warnings.simplefilter('ignore', RuntimeWarning)
        quiet = PR.posterior_predictive(pm, chain, days=[2], reweight={'flat': rw['flat'], 'options': dict(min_ess=5)})
    assert quiet.reweight.members('flat') == 4
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with pytest.raises(ValueError, match="'gone'"):
            PR.posterior_predictive(pm, chain, days=[2], reweight={'gone': dict(log_weights=[np.full(12, -INF)]),
                                                                   'flat': rw['flat']})
    pm.close()


def test_without_reweight_nothing_changes(tmp_path):
    from parasitoids_amd import predictive as PR
    pm = _pop_model()
    trace, names = _chain([2, 1])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        res = PR.posterior_predictive(pm, (trace, names), thresholds=THR)
    assert res.reweight is None and res.reweight_info is None
    res.save(str(tmp_path / 'p' / 'pp'))
    assert sorted(os.listdir(str(tmp_path / 'p'))) == ['pp.json', 'pp.npz']
    assert 'reweight' not in json.load(open(str(tmp_path / 'p' / 'pp.json')))['predictive']
    pm.close()
