"""GPU tests of the release plans (ps_sites_*, predictive.ReleaseSites) and of the accumulators fed from them
(SpreadSummary / SpreadHistogram / ArrivalMaps .for_projection): the device fields bit for bit against the numpy
reference (sites_ref.plan_fields of `PopModel.population(d)`), plumes that leave the domain, staggered release
days with a model of their own, the call order of the groups, the posterior of a sum against the sum of
posteriors, add and merge order, the untouched day-based paths, posterior_predictive with sites=, and the
refusals of the C ABI.  Kalbar wind, R = 64 and 128, 6 days, the members and weights of test_projection_gpu.py."""
import ctypes as C
import json
import os
import warnings

import numpy as np
import pytest

import arrival_ref
from helpers import HP, DP, DLP, MU_R, NPER
from hist_ref import weighted_counts
from sites_ref import plan_fields, shifted

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.abspath(__file__))
MEMBERS = [(DP, MU_R), ((160.0, 150.0, 0.2), 1.1), ((185.0, 140.0, 0.3), 1.25), ((171.82, 160.0, 0.1), 1.0),
           ((150.0, 135.0, 0.28), 1.15)]
WEIGHTS = [1, 3, 1, 2, 1]
THR = [1.0, 10.0]
DAYS = list(range(6))
OUT = [0, 1, 2, 3, 5]


def _wind():
    from parasitoids_amd import ParasitoidModel as PM
    return PM.get_wind_data(os.path.join(ROOT, 'golden', 'data', 'kalbar'), 30, '00:00')


def _pop_model(R=64, first=0, ndays=6, **kw):
    from parasitoids_amd.pop_model import PopModel
    wd, days = _wind()
    return PopModel(wd, days[first:ndays], domain_info=(10000.0, R), r_number=130000, **kw)


def _evaluate(pm, member, **kw):
    dp, mu = member
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        pm.evaluate(HP, dp, DLP, mu, NPER, want_stats=False, **kw)


def _fields(pm):
    return np.array([pm.population(d).toarray() for d in range(pm._nd)])


def _metres(cells, R):
    """(drow, dcol, amount, lag) in cells -> (east_m, north_m, amount, lag); the cell size is a power of two
    times 5^4, so the way back is exact"""
    res = 10000.0 / R
    return [(dc * res, -dr * res, a, lag) for dr, dc, a, lag in cells]


def _edge_plan(R):
    """site (0, 0); an odd and an even column offset, one with a negative row offset; two sites on one cell; a
    site one cell from the east edge and one one cell from the north edge"""
    return [(0, 0, 1.0, 0), (-5, 3, 0.5, 0), (7, -4, 0.25, 0), (7, -4, 0.125, 0), (2, R - 1, 0.3, 0),
            (-(R - 1), -2, 0.2, 0)]


STAGGERED = [(0, 0, 0.6, 0), (0, 13, 0.4, 0), (9, -6, 0.5, 2)]     # 60 % here, 40 % east, a third batch later, south


def _flat_wrapped(f, drow, dcol):
    """the wrong translation: the flat index shifted and tested against the flat range only"""
    n = f.shape[0]
    out = np.zeros(f.size)
    s = drow * n + dcol
    src = np.arange(f.size) - s
    ok = (src >= 0) & (src < f.size)
    out[ok] = f.ravel()[src[ok]]
    return out.reshape(f.shape)


@pytest.mark.parametrize('R, prob_model, mode', [(64, False, 'exact'), (64, True, 'exact'), (64, False, None),
                                                 (64, True, None), (128, False, None), (128, True, 'exact')])
def test_device_fields_match_the_numpy_reference_bit_for_bit(R, prob_model, mode):
    from parasitoids_amd.predictive import ReleaseSites
    pm = _pop_model(R, prob_model=prob_model, **({} if mode is None else {'mode': mode}))
    cells = _edge_plan(R)
    N = 2 * R + 1
    with ReleaseSites(pm, _metres(cells, R)) as P:
        assert P.N == N and P.nout == 6 and P.days == DAYS and P.lags == [0] and P.live == DAYS
        assert [(s['drow'], s['dcol']) for s in P.sites] == [c[:2] for c in cells]
        assert P.nbytes == 6 * ((N * N + 63) // 64 * 64) * 8
        for n, mem in enumerate(MEMBERS[:2]):              # the second apply overwrites the first
            _evaluate(pm, mem)
            P.apply()
            f = _fields(pm)
            ref = plan_fields({0: f}, cells, DAYS)
            # the reference itself loses mass over the east and the north edge and is non-zero along them,
            # so a translation that wraps would change a bit
            assert ref[..., -1].max() > 0 and ref[:, 0, :].max() > 0
            for dr, dc, _a, _lag in cells[4:]:
                assert shifted(f[5], dr, dc).sum() < 0.9 * f[5].sum()
            wrapped = ref[5] - 0.3 * shifted(f[5], 2, R - 1) + 0.3 * _flat_wrapped(f[5], 2, R - 1)
            assert np.abs(wrapped[:, 0] - ref[5][:, 0]).max() > 0
            for e in range(6):
                got = P.field(e)
                assert got.dtype == np.float64 and got.shape == (N, N)
                assert np.array_equal(got, ref[e]), (n, e, np.abs(got - ref[e]).max())
                assert not np.signbit(got).any()
                # column 0 of the rows below the plume that left east holds what the reference holds
                assert np.array_equal(got[:, 0], ref[e][:, 0]) and np.array_equal(got[:, -1], ref[e][:, -1])
            assert np.array_equal(P.field(0)[R - 5:R + 8, R - 4:R + 4], ref[0][R - 5:R + 8, R - 4:R + 4])
        assert P.applies == 2
        # the tail cell, its neighbour, the centre, and the pairs that straddle a row end (flat index even)
        rows = np.array([N - 1, N - 1, R, 2, 3, 3, 4, 0, 0])
        cols = np.array([N - 1, N - 2, R, N - 1, 0, N - 1, 0, 0, N - 1])
        g = P.gather(rows, cols)
        assert g.shape == (6, 9) and g[:, 0].max() >= 0 and g[5].max() > 0
        assert np.array_equal(g, np.array([P.field(e)[rows, cols] for e in range(6)]))
        assert np.array_equal(g, ref[:, rows, cols])
    pm.close()


def _state_error(rc, lib):
    from parasitoids_amd import _lib as L
    assert rc == L.PS_ERR_STATE, (rc, lib.ps_last_error())


def test_staggered_release_days_and_the_order_of_the_groups():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import ArrivalMaps, ReleaseSites, SpreadHistogram, SpreadSummary, lagged_models
    R = 64
    pm = _pop_model(R)
    late = lagged_models(pm, [0, 2])
    assert list(late) == [2] and late[2].days == pm.days[2:] and late[2].r_number == pm.r_number
    with pytest.raises(ValueError, match='no model for the release 2 days'):
        ReleaseSites(pm, _metres(STAGGERED, R), OUT)
    with ReleaseSites(pm, _metres(STAGGERED, R), OUT, late) as P, \
            ReleaseSites(pm, _metres(STAGGERED[:2], R), OUT) as P0, SpreadSummary.for_projection(P) as S, \
            SpreadHistogram.for_projection(P) as H, ArrivalMaps.for_projection(P, THR) as A:
        lib = P._lib
        assert P.lags == [0, 2] and P.groups == [(0, [0, 1]), (2, [2])] and A.days == OUT and S.days == list(range(5))
        assert P.slots == [[0, 1, 2, 3, 5], [None, None, 0, 1, 3]]
        with pytest.raises(ValueError, match='release plan'):
            P.apply()                                      # nothing evaluated yet
        _evaluate(pm, MEMBERS[1])
        with pytest.raises(ValueError, match=r'release plan \(lag 2\)'):
            P.apply()                                      # the later release's model neither: nothing applied
        assert P.applies == 0
        _evaluate(late[2], MEMBERS[1], ndays=4)
        P.profile(True)
        calls = P._calls()
        assert list(calls[1][3][:5]) == [L.REC_NONE, L.REC_NONE, L.REC_STATE, L.REC_CHAIN, L.REC_CHAIN]
        _state_error(lib.ps_sites_apply(P._h, *calls[1]), lib)          # group 1 before group 0
        out = np.empty((P.N, P.N))
        _state_error(lib.ps_sites_fetch(P._h, 0, L.p_f64(out)), lib)    # nothing applied yet
        L.check(lib.ps_sites_apply(P._h, *calls[0]))
        _state_error(lib.ps_sites_fetch(P._h, 0, L.p_f64(out)), lib)    # between the groups
        assert b'group 1 of 2' in lib.ps_last_error()
        with pytest.raises(L.HipError) as err:
            P.gather([0], [0])
        assert err.value.code == L.PS_ERR_STATE
        for acc in (S, H, A):
            with pytest.raises(L.HipError) as err:
                acc.add(1)
            assert err.value.code == L.PS_ERR_STATE and acc.members == 0 and acc.total_weight == 0
        assert P.profile()[1] == 1 and P.applies == 0                   # nothing but group 0 was enqueued
        L.check(lib.ps_sites_apply(P._h, *calls[1]))
        assert P.applies == 1 and P.profile()[1] == 2
        f0, f2 = _fields(pm), _fields(late[2])
        assert f0.shape[0] == 6 and f2.shape[0] == 4
        ref = plan_fields({0: f0, 2: f2}, STAGGERED, OUT)
        got = np.array([P.field(e) for e in range(5)])
        assert np.array_equal(got, ref)
        # before day 2 the plan is its day-0 sites alone; from day 2 on the later batch shows
        P0.apply()
        for e in (0, 1):
            assert np.array_equal(got[e], P0.field(e))
        for e in (2, 3, 4):
            assert (got[e] - P0.field(e)).max() > 1.0
        # a whole pass through apply(), another member: overwritten, and the accumulators take it
        _evaluate(pm, MEMBERS[0])
        _evaluate(late[2], MEMBERS[0], ndays=4)
        P.apply()
        ref = plan_fields({0: _fields(pm), 2: _fields(late[2])}, STAGGERED, OUT)
        assert np.array_equal(np.array([P.field(e) for e in range(5)]), ref)
        for acc in (S, H, A):
            acc.add(2)
        assert np.array_equal(S.mean(4), ref[4]) and not S.variance(4).any()
        assert np.array_equal(H.counts(2).astype(np.int64), weighted_counts([ref[2]], [2], H.edges))
        assert np.array_equal(A.counts(0, 2).astype(np.int64), arrival_ref.weighted_counts([ref], [2], THR)[0, 2])
        # group 0 may open a new pass at any time; the pass then has to be finished again
        calls = P._calls()
        L.check(lib.ps_sites_apply(P._h, *calls[0]))
        L.check(lib.ps_sites_apply(P._h, *calls[0]))
        _state_error(lib.ps_summary_add_sites(S._h, P._h, 1), lib)                 # the new pass is under way
        L.check(lib.ps_sites_apply(P._h, *calls[1]))
        assert np.array_equal(P.field(3), ref[3]) and S.members == 1
    for m in (pm, late[2]):
        m.close()


def _weighted_moments(Y, weights):
    """Y: [member, ...] -> (mean, population variance) with integer weights"""
    w = np.asarray(weights, dtype=np.float64).reshape((-1,) + (1,) * (Y.ndim - 1))
    mean = (w * Y).sum(0) / w.sum()
    return mean, (w * (Y - mean) ** 2).sum(0) / w.sum()


def test_posterior_of_the_sum_over_sites():
    """summary, histogram and arrival maps of the plan over five weighted members against the same statistics of
    the members' reference plan fields; the sum of the per-site variances is another number; neither the order
    of the adds nor that of the merges changes a bit of the integer accumulators"""
    from parasitoids_amd.predictive import ArrivalMaps, ReleaseSites, SpreadHistogram, SpreadSummary, lagged_models
    R = 64
    out = [0, 2, 5]
    pm = _pop_model(R)
    late = lagged_models(pm, [2])
    Y, parts = [], []
    with ReleaseSites(pm, _metres(STAGGERED, R), out, late) as P:
        S = [SpreadSummary.for_projection(P, THR) for _ in range(4)]
        H = [SpreadHistogram.for_projection(P) for _ in range(4)]
        A = [ArrivalMaps.for_projection(P, THR) for _ in range(4)]
        order = list(range(len(MEMBERS)))
        for i in order + order[::-1]:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)
                P.evaluate(HP, MEMBERS[i][0], DLP, MEMBERS[i][1], NPER)
            first = len(Y) < len(MEMBERS)
            for acc in (S, H, A):
                if first:
                    acc[0].add(WEIGHTS[i])
                    acc[2 if i < 2 else 3].add(WEIGHTS[i])
                else:
                    acc[1].add(WEIGHTS[i])
            if first:
                fields = {0: _fields(pm), 2: _fields(late[2])}
                Y.append(plan_fields(fields, STAGGERED, out))
                parts.append([plan_fields(fields, [s], out) for s in STAGGERED])      # every site alone
        Y = np.array(Y)                                    # [member, output, N, N]
        Wt = float(sum(WEIGHTS))
        assert S[0].total_weight == Wt and S[0].members == len(MEMBERS) and A[0].days == out
        mean, var = _weighted_moments(Y, WEIGHTS)
        for e in range(3):
            np.testing.assert_allclose(S[0].mean(e), mean[e], rtol=1e-12, atol=1e-12 * mean[e].max())
            np.testing.assert_allclose(S[0].variance(e), var[e], rtol=1e-9, atol=1e-12 * var[e].max())
            for k, t in enumerate(THR):
                cnt = sum(w * (y >= t).astype(np.int64) for w, y in zip(WEIGHTS, Y[:, e]))
                assert 0 < cnt.max() <= Wt
                assert np.array_equal(S[0].exceedance(e, k), cnt.astype(np.float64) / Wt)
            got = H[0].counts(e)
            assert got.dtype == np.uint32
            assert np.array_equal(got.astype(np.int64), weighted_counts(Y[:, e], WEIGHTS, H[0].edges)), e
        # the sites share the member's parameters, so where their plumes overlap the fields move together: the
        # variance of the sum is not the sum of the per-site variances (looked at where the two differ most)
        per_site = sum(_weighted_moments(np.array([p[k][2] for p in parts]), WEIGHTS)[1] for k in range(3))
        c = np.unravel_index(np.argmax(np.abs(var[2] - per_site)), var[2].shape)
        assert abs(S[0].variance(2)[c] - per_site[c]) > 0.01 * var[2][c] > 0, (var[2][c], per_site[c])
        ref_cnt = arrival_ref.weighted_counts(list(Y), WEIGHTS, THR)       # [K, nslot + 1, N, N]
        rows = arrival_ref.reached_rows(list(Y), THR)
        for k in range(len(THR)):
            for s, d in enumerate(out + [None]):
                assert np.array_equal(A[0].counts(k, d).astype(np.int64), ref_cnt[k, s]), (k, d)
            cells, w = A[0].reached(k)
            assert np.array_equal(cells, rows[:, k]) and list(w) == WEIGHTS
            assert 0 < rows[0, k, 0] < rows[0, k, 2]
        area = A[0].reached_area(1, (0.5,))
        assert [a['day'] for a in area] == out
        assert area[2]['quantiles'][0] == arrival_ref.area_quantile(rows[:, 1, 2], WEIGHTS, 0.5) * (10000.0 / R) ** 2
        # add order (reversed) and merge order (second half + first half, first half + second half)
        S[3].merge(S[2])
        H[2].merge(H[3])
        A[2].merge(A[3])
        for e in range(3):
            c0 = H[0].counts(e)
            assert np.array_equal(H[1].counts(e), c0) and np.array_equal(H[2].counts(e), c0)
            for other in (S[1], S[3]):
                for k in range(len(THR)):
                    assert np.array_equal(other.exceedance(e, k), S[0].exceedance(e, k))
                np.testing.assert_allclose(other.mean(e), mean[e], rtol=1e-12, atol=1e-12 * mean[e].max())
        for k in range(len(THR)):
            for d in out + [None]:
                c0 = A[0].counts(k, d)
                assert np.array_equal(A[1].counts(k, d), c0) and np.array_equal(A[2].counts(k, d), c0)
            assert np.array_equal(A[1].reached(k)[0], A[0].reached(k)[0][::-1])
            assert np.array_equal(A[2].reached(k)[0], A[0].reached(k)[0])
            assert np.array_equal(A[2].quantile(k, 0.5), A[0].quantile(k, 0.5))
        for a in S + H + A:
            a.close()
    for m in (pm, late[2]):
        m.close()


def _all_maps(S, H, A, SP, days, nthr):
    out = []
    for d in days:
        out += [S.mean(d), S.variance(d)] + [S.exceedance(d, k) for k in range(nthr)]
        out += [H.counts(d), H.quantile(d, 0.5)]
        out += [A.counts(k, d) for k in range(nthr)]
    out += [A.quantile(k, 0.5) for k in range(nthr)] + [A.reached(k)[0] for k in range(nthr)]
    out += [SP.mean(e) for e in range(3)] + [SP.variance(e) for e in range(3)]
    return out


def test_day_based_and_projection_fed_accumulators_are_untouched_by_a_plan():
    """each pass starts from fresh models: an auto-mode model routes days by what it has seen before, which may
    move a field by rounding"""
    from parasitoids_amd.predictive import (ArrivalMaps, Projection, ReleaseSites, SpreadHistogram, SpreadSummary,
                                            exposure_weights)
    R = 64
    days = [0, 3, 5]
    W = exposure_weights(DAYS, [0, 2, 5])
    passes = []
    for with_plan in (False, True):
        pm = _pop_model(R)
        with SpreadSummary(pm, days, THR) as S, SpreadHistogram(pm, days) as H, ArrivalMaps(pm, THR, days) as A, \
                Projection(pm, W, DAYS) as X, SpreadSummary.for_projection(X, THR) as SP:
            plan = []
            if with_plan:
                P = ReleaseSites.with_lagged_models(pm, _metres(STAGGERED, R), OUT)
                plan = [P, SpreadSummary.for_projection(P, THR), SpreadHistogram.for_projection(P),
                        ArrivalMaps.for_projection(P, THR), ArrivalMaps.for_projection(X, THR)]
            for mem, w in zip(MEMBERS, WEIGHTS):
                _evaluate(pm, mem)
                if with_plan:
                    with warnings.catch_warnings():
                        warnings.simplefilter('ignore', RuntimeWarning)
                        P.evaluate_lagged(HP, mem[0], DLP, mem[1], NPER)
                S.add(w)
                if with_plan:
                    P.apply()
                    plan[1].add(w)
                H.add(w)
                X.apply()
                if with_plan:
                    plan[2].add(w)
                    plan[4].add(w)
                SP.add(w)
                A.add(w)
                if with_plan:
                    plan[3].add(w)
            passes.append(_all_maps(S, H, A, SP, days, len(THR)))
            if with_plan:
                assert plan[1].total_weight == plan[3].total_weight == S.total_weight == sum(WEIGHTS)
                # arrival maps of a projection: the slots are its outputs, here the exposure up to days 0, 2, 5
                assert plan[4].days == [0, 1, 2] and plan[4].members == len(MEMBERS)
                assert plan[4].counts(0, 0).max() > 0 and plan[1].mean(4).max() > 0
            for a in plan[::-1]:
                a.close()
        pm.close()
    assert len(passes[0]) == len(passes[1])
    for a, b in zip(*passes):
        assert np.array_equal(a, b)


def test_arrival_maps_of_a_projection_match_the_reference():
    from parasitoids_amd.predictive import ArrivalMaps, Projection, exposure_weights
    from project_ref import project
    pm = _pop_model(64)
    W = np.concatenate([exposure_weights(DAYS, [0, 2]), np.zeros((1, 6)), exposure_weights(DAYS, [5])])
    Y = []
    with Projection(pm, W, DAYS) as X, ArrivalMaps.for_projection(X, [50.0, 500.0]) as A:
        assert X.live == [0, 1, 3] and A.days == [0, 1, 3]      # the output without weight has no slot
        for mem, w in zip(MEMBERS[:3], WEIGHTS[:3]):
            _evaluate(pm, mem)
            X.apply()
            A.add(w)
            Y.append(project(_fields(pm), W)[[0, 1, 3]])
        ref = arrival_ref.weighted_counts(Y, WEIGHTS[:3], A.thresholds)
        for k in range(2):
            for s, d in enumerate([0, 1, 3, None]):
                assert np.array_equal(A.counts(k, d).astype(np.int64), ref[k, s]), (k, d)
            assert np.array_equal(A.reached(k)[0], arrival_ref.reached_rows(Y, A.thresholds)[:, k])
        assert ref[1, 1].max() > 0 and ref[1, 2].max() > 0
    pm.close()


def _csr(f, key, N):
    from scipy import sparse
    return sparse.csr_matrix((f[key + '_data'], f[key + '_ind'], f[key + '_indptr']), shape=(N, N)).toarray()


def _chain(rng_rows):
    """a short synthetic chain: runs of identical model parameters around the sampler's start values"""
    from parasitoids_amd import mcmc
    names = [m[0] for m in mcmc.MODEL_BLOCK]
    base = np.array([m[2] for m in mcmc.MODEL_BLOCK], dtype=np.float64)
    rows = []
    for n, length in enumerate(rng_rows):
        t = base.copy()
        t[names.index('sig_x')] += 6.0 * n
        t[names.index('sig_y')] -= 4.0 * n
        t[names.index('mu_r')] += 0.03 * n
        rows += [t] * length
    return np.array(rows), names


def test_posterior_predictive_with_a_release_plan(tmp_path, monkeypatch):
    from parasitoids_amd import mcmc
    from parasitoids_amd import predictive as PR
    R, N = 64, 129
    trace, names = _chain([2, 1, 3, 1, 2])
    chains = [(trace[:5], names), (trace[5:], names)]       # the run of three is cut in two: 2 + 1 + 2 | 1 + 1 + 2
    arg = dict(sites=[s[:3] + ((s[3],) if s[3] else ()) for s in _metres(STAGGERED, R)], days=OUT)
    kw = dict(thresholds=(1.0,), quantiles=[0.5], arrival=THR, arrival_levels=(0.5,))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        pa, pb = _pop_model(R, mode='exact'), _pop_model(R, mode='exact')
        res = PR.posterior_predictive(pa, chains, sites=arg, **kw)
        plain = PR.posterior_predictive(pb, chains, **kw)
        with pytest.raises(ValueError, match="beyond the model's 6 days"):
            PR.posterior_predictive(pb, chains, sites=dict(sites=[(0, 0, 1), (0, 0, 1, 7)]), **kw)
    assert plain.sites is None and res.failed == 0 and res.evaluations == 6 and len(res.runs) == 6
    st = res.sites
    assert st.labels == OUT and st.weights is None and st.plan['lags'] == [0, 2] and st.plan['days'] == OUT
    assert [(s['drow'], s['dcol'], s['amount'], s['lag']) for s in st.plan['sites']] == STAGGERED
    for acc in (st.summary, st.histogram, st.arrival):
        assert acc.total_weight == res.summary.total_weight == 9 and acc.members == res.summary.members == 6
    # by hand: every run once more through the classes, and through the numpy reference
    cols = [names.index(m[0]) for m in mcmc.MODEL_BLOCK]
    pm = _pop_model(R, mode='exact')
    Y, W = [], []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        with PR.ReleaseSites.with_lagged_models(pm, arg['sites'], OUT) as P, \
                PR.SpreadSummary.for_projection(P, (1.0,)) as S, PR.SpreadHistogram.for_projection(P) as H, \
                PR.ArrivalMaps.for_projection(P, THR) as A:
            for ci, first, weight in res.runs:
                P.evaluate(*mcmc.model_args(chains[ci][0][first, cols]))
                for acc in (S, H, A):
                    acc.add(weight)
                Y.append(plan_fields({0: _fields(pm), 2: _fields(P.lagged[2])}, STAGGERED, OUT))
                W.append(weight)
            mean, _var = _weighted_moments(np.array(Y), W)
            for e in range(5):
                np.testing.assert_allclose(st.summary.mean(e), S.mean(e), rtol=1e-12, atol=1e-12 * mean[e].max())
                np.testing.assert_allclose(st.summary.mean(e), mean[e], rtol=1e-12, atol=1e-12 * mean[e].max())
                assert np.array_equal(st.summary.exceedance(e, 0), S.exceedance(e, 0))
                assert np.array_equal(st.histogram.counts(e), H.counts(e))
            for k in range(2):
                for d in OUT + [None]:
                    assert np.array_equal(st.arrival.counts(k, d), A.counts(k, d))
                assert np.array_equal(st.arrival.reached(k)[0], A.reached(k)[0])
                assert np.array_equal(A.reached(k)[0], arrival_ref.reached_rows(Y, THR)[:, k])
    npz, js = res.save(str(tmp_path / 'a' / 'pp'))
    npz_p, js_p = plain.save(str(tmp_path / 'p' / 'pp'))
    assert not os.path.exists(str(tmp_path / 'p' / 'pp_sites.npz'))
    with np.load(npz) as fa, np.load(npz_p) as fp:          # the main file does not know about the plan
        assert set(fa.files) == set(fp.files)
        for key in fp.files:
            assert np.array_equal(fa[key], fp[key]), key
    with np.load(str(tmp_path / 'a' / 'pp_sites.npz')) as fz:
        assert [int(x) for x in fz['days']] == OUT
        want = {'days', 'arrival0_q50', 'arrival1_q50', 'arrival0_cells', 'arrival1_cells', 'arrival_weights'}
        for e, lab in enumerate(OUT):
            for suffix, m in (('', st.summary.mean(e)), ('_sd', st.summary.sd(e)),
                              ('_pexc0', st.summary.exceedance(e, 0)), ('_q50', st.histogram.quantile(e, 0.5)),
                              ('_parr0', st.arrival.prob_by(0, lab)), ('_parr1', st.arrival.prob_by(1, lab))):
                assert np.array_equal(_csr(fz, '%d%s' % (lab, suffix), N), np.where(m >= 1e-8, m, 0.0)), (lab, suffix)
                want |= {'%d%s_%s' % (lab, suffix, t) for t in ('data', 'ind', 'indptr')}
        assert set(fz.files) == want
        assert np.array_equal(fz['arrival1_q50'], st.arrival.quantile(1, 0.5)) and fz['arrival1_q50'].dtype == np.int16
        assert np.array_equal(fz['arrival0_cells'], st.arrival.reached(0)[0]) and list(fz['arrival_weights']) == W
    meta = json.load(open(js))['predictive']
    ms = meta['sites']
    assert ms['lags'] == [0, 2] and ms['days'] == OUT and ms['labels'] == OUT and ms['thresholds'] == [1.0]
    assert [(s['drow'], s['dcol']) for s in ms['sites']] == [s[:2] for s in STAGGERED]
    assert [(s['east'], s['north'], s['amount'], s['lag']) for s in ms['sites']] == [tuple(s) for s in _metres(STAGGERED, R)]
    assert ms['arrival']['thresholds'] == THR and len(ms['arrival']['reached_area']) == 2
    assert [a['day'] for a in ms['arrival']['reached_area'][0]] == OUT
    assert ms['arrival']['reached_area'][1] == st.arrival.reached_area(1, (0.5,))
    assert 'sites' not in json.load(open(js_p))['predictive']
    # a later release's model that fails for one member leaves that member out of every accumulator
    real = PR.lagged_models
    seen = []

    def failing(pop_model, lags, wind_data=None):
        made = real(pop_model, lags, wind_data)
        inner = made[2].evaluate

        def evaluate(*a, **k):
            seen.append(1)
            if len(seen) == 2:
                raise ValueError('no kernel for this member')
            return inner(*a, **k)
        made[2].evaluate = evaluate
        return made
    monkeypatch.setattr(PR, 'lagged_models', failing)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        pc = _pop_model(R, mode='exact')
        part = PR.posterior_predictive(pc, chains[:1], sites=arg, **kw)
    assert part.failed == 1 and part.evaluations == 3 and [r[1:] for r in part.runs] == [(0, 2), (3, 2)]
    for acc in (part.summary, part.histogram, part.arrival, part.sites.summary, part.sites.histogram,
                part.sites.arrival):
        assert acc.members == 2 and acc.total_weight == 4
    for e in range(5):
        ref = (2 * Y[0][e] + 2 * Y[2][e]) / 4.0
        np.testing.assert_allclose(part.sites.summary.mean(e), ref, rtol=1e-12, atol=1e-12 * ref.max())
    for r in (res, plain, part):
        for acc in (r.summary, r.histogram, r.arrival, r.sites):
            if acc is not None:
                acc.close()
    for p in (pm, pa, pb, pc):
        p.close()


def test_refusals_at_the_c_abi_and_the_handles_stay_usable():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import (NEGVAL, ArrivalMaps, CatchFields, ReleaseSites, SpreadHistogram,
                                            SpreadSummary, _day_scales)
    lib = L.load()
    dev = L.default_device()
    h = L._VP()

    def create(groups, drow, dcol, amount, N=129, nout=3, device=dev):
        return lib.ps_sites_create(device, N, nout, len(groups), L.p_i32(L.i32(groups)), L.p_i32(L.i32(drow)),
                                   L.p_i32(L.i32(dcol)), L.p_f64(L.f64(amount)), C.byref(h))
    one = ([1], [0], [0], [1.0])
    assert create(*one, nout=0) == L.PS_ERR_BAD_ARG and not h
    assert create(*one, nout=33) == L.PS_ERR_BAD_ARG and not h
    assert create([1] * 9, [0] * 9, [0] * 9, [1.0] * 9) == L.PS_ERR_BAD_ARG and not h
    assert create([], [], [], []) == L.PS_ERR_BAD_ARG and not h
    assert create([1, 0], [0], [0], [1.0]) == L.PS_ERR_BAD_ARG and not h
    assert b'group 1 has 0 sites' in lib.ps_last_error()
    assert create([20, 13], [0] * 33, [0] * 33, [1.0] * 33) == L.PS_ERR_BAD_ARG and not h
    assert b'more than 32 sites' in lib.ps_last_error()
    for dr, dc in ((129, 0), (0, -129)):
        assert create([1], [dr], [dc], [1.0]) == L.PS_ERR_BAD_ARG and not h
        assert b'site 0 is offset' in lib.ps_last_error()
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert create([2], [0, 0], [0, 0], [1.0, bad]) == L.PS_ERR_BAD_ARG and not h
        assert b'amount 1' in lib.ps_last_error()
    assert create(*one, device=99) == L.PS_ERR_NO_DEVICE and not h
    assert create(*one, N=60001, nout=32) == L.PS_ERR_OOM and not h           # 0.9 TB of outputs
    assert b'GB free' in lib.ps_last_error()
    assert create([1], [128], [-128], [1.0]) == L.PS_OK and h                  # |offset| = N - 1 is allowed
    lib.ps_sites_destroy(h)
    pm, big = _pop_model(64), _pop_model(128)
    cells = [(0, 0, 1.0, 0), (3, 5, 0.5, 0)]
    with ReleaseSites(pm, _metres(cells, 64), [0, 2, 5]) as P, ReleaseSites(big, _metres(cells, 128), [0, 2, 5]) as P128, \
            SpreadSummary.for_projection(P, THR) as S, SpreadHistogram.for_projection(P) as H, \
            ArrivalMaps.for_projection(P, THR) as A, SpreadSummary(pm, [0, 1]) as S2, \
            SpreadHistogram(pm, [0, 1]) as H2, ArrivalMaps(pm, THR, [0, 1]) as A2, \
            CatchFields(pm, [(0, 1.0), (1, 1.0)]) as CF:
        _evaluate(pm, MEMBERS[0])
        _evaluate(big, MEMBERS[0])
        P.profile(True)
        call = list(P._calls()[0])
        wrong = list(call)
        wrong[0] = big.solver._h
        assert lib.ps_sites_apply(P._h, *wrong) == L.PS_ERR_BAD_ARG               # a solver of another domain
        assert lib.ps_last_error() == b'sites_apply: solver domain 257, handle domain 129'
        # the same refusal, word for word, of an add and of an apply over the day records of that solver
        stat, post = _day_scales(big, [0, 1])

        def records(h):
            return (h._h, big.solver._h, 2, L.p_i32(h._kind), L.p_i32(h._idx), L.p_f64(stat), L.p_f64(post),
                    L.p_i32(h._delta), NEGVAL)
        assert lib.ps_summary_add(*records(S2), 1) == L.PS_ERR_BAD_ARG
        assert lib.ps_last_error() == b'summary_add: solver domain 257, summary domain 129'
        assert lib.ps_catch_apply(*records(CF)) == L.PS_ERR_BAD_ARG
        assert lib.ps_last_error() == b'catch_apply: solver domain 257, handle domain 129'
        assert CF.applies == 0
        wrong = list(call)
        wrong[2] = 2
        assert lib.ps_sites_apply(P._h, *wrong) == L.PS_ERR_BAD_ARG               # two slots for three outputs
        wrong = list(call)
        wrong[1] = 1
        assert lib.ps_sites_apply(P._h, *wrong) == L.PS_ERR_BAD_ARG               # the plan has one group
        wrong = list(call)
        wrong[4] = L.p_i32(L.i32([0, 1, 999]))
        assert lib.ps_sites_apply(P._h, *wrong) != L.PS_OK                        # a record the run does not have
        wrong = list(call)
        wrong[3] = L.p_i32(L.i32([L.REC_NONE] * 3))
        assert lib.ps_sites_apply(P._h, *wrong) == L.PS_ERR_BAD_ARG               # a group released on no output day
        assert P.applies == 0 and P.profile()[1] == 0                             # nothing was enqueued
        with pytest.raises(L.HipError) as err:
            P.field(0)
        assert err.value.code == L.PS_ERR_STATE
        P.apply()
        P128.apply()
        # slot count: 3 outputs into 2 slots; domain: 257 x 257 outputs into 129 x 129 slots; weight 0
        for fn, small, right in ((lib.ps_summary_add_sites, S2, S), (lib.ps_hist_add_sites, H2, H),
                                 (lib.ps_arrival_add_sites, A2, A)):
            assert fn(small._h, P._h, 1) == L.PS_ERR_BAD_ARG
            assert b'release plan has 3 outputs' in lib.ps_last_error()
            assert fn(right._h, P128._h, 1) == L.PS_ERR_BAD_ARG
            assert fn(right._h, P._h, 0) == L.PS_ERR_BAD_ARG
            assert fn(right._h, None, 1) == L.PS_ERR_BAD_ARG
        with pytest.raises(L.HipError):
            P.gather([129], [0])                           # a cell outside the domain
        with pytest.raises(ValueError):
            P.field(3)
        for acc in (S, H, A, S2, H2, A2):
            assert acc.members == 0 and acc.total_weight == 0
        # every handle still works
        ref = plan_fields({0: _fields(pm)}, cells, [0, 2, 5])
        for e in range(3):
            assert np.array_equal(P.field(e), ref[e])
        for acc in (S, H, A, S2):
            acc.add(2)
        assert S.members == 1 and S.total_weight == 2 and A.total_weight == 2
        assert np.array_equal(S.mean(2), ref[2]) and np.array_equal(S2.mean(1), _fields(pm)[1])
        assert np.array_equal(A.counts(1, 5).astype(np.int64), arrival_ref.weighted_counts([ref], [2], THR)[1, 2])
        N, nout, ng, ns, passes = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        L.check(lib.ps_sites_info(P._h, C.byref(N), C.byref(nout), C.byref(ng), C.byref(ns), C.byref(passes)))
        assert (N.value, nout.value, ng.value, ns.value, passes.value) == (129, 3, 1, 2, 1)
    pm.close()
    big.close()
