"""GPU tests of the posterior sensitivity maps (ps_sens_*, predictive.SensitivityMaps): the device mean and
co-moments bit for bit against the numpy replay (sens_ref.add of `PopModel.population(d)`), mean and M2 bit for
bit against a SpreadSummary fed alongside, the covariance maps against a numpy two-pass, weights and merging, the
properties of the correlation maps, the finalize against its replay, projections and release plans as sources,
the untouched accumulators, posterior_predictive with sensitivity= and its saved files, and the refusals of the
C ABI.  Kalbar wind, R = 128 (N = 257: N * N is odd and the pitch differs from it), 6 days, the members and
weights of test_predictive_gpu.py."""
import contextlib
import ctypes as C
import json
import os
import warnings

import numpy as np
import pytest
from scipy import sparse

import sens_ref
from helpers import HP, DP, DLP, MU_R, NPER

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.abspath(__file__))
MEMBERS = [(DP, MU_R), ((160.0, 150.0, 0.2), 1.1), ((185.0, 140.0, 0.3), 1.25), ((171.82, 160.0, 0.1), 1.0),
           ((150.0, 135.0, 0.28), 1.15)]
WEIGHTS = [1, 3, 1, 2, 1]
DAYS = list(range(6))
THREE = ['sig_x', 'sig_y', 'mu_r']
N = 257


def _wind():
    from parasitoids_amd import ParasitoidModel as PM
    return PM.get_wind_data(os.path.join(ROOT, 'golden', 'data', 'kalbar'), 30, '00:00')


def _pop_model(R=128, first=0, ndays=6, **kw):
    from parasitoids_amd.pop_model import PopModel
    wd, days = _wind()
    return PopModel(wd, days[first:ndays], domain_info=(10000.0, R), r_number=130000, **kw)


def _evaluate(pm, member, **kw):
    dp, mu = member
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        pm.evaluate(HP, dp, DLP, mu, NPER, want_stats=False, **kw)


def _fields(pm, days=DAYS):
    return np.array([pm.population(d).toarray() for d in days])


def _names():
    from parasitoids_amd import mcmc
    return [m[0] for m in mcmc.MODEL_BLOCK]


def _member_trace(mems, repeats):
    from parasitoids_amd import mcmc
    t0 = np.array([m[2] for m in mcmc.MODEL_BLOCK])
    names = _names()
    rows = []
    for (dp, mu), n in zip(mems, repeats):
        t = t0.copy()
        t[names.index('sig_x')], t[names.index('sig_y')], t[names.index('corr_p')] = dp[0], dp[1], (dp[2] + 1) / 2
        t[names.index('mu_r')] = mu
        rows += [t] * n
    return np.array(rows), names


def _thetas(mems=MEMBERS):
    return _member_trace(mems, [1] * len(mems))[0]


def _cols(params):
    names = _names()
    return [names.index(p) for p in (names if params is None else params)]


def _scale_sd(mean, T, w, cols):
    """the scale of the fields and the posterior sd of every listed scalar: what the tolerances are relative to"""
    w = np.asarray(w, dtype=float)
    Tm = T[:, cols]
    sd = np.sqrt(w @ (Tm - w @ Tm / w.sum()) ** 2 / w.sum())
    return np.abs(mean).max(), sd


def _cov(H, d):
    return np.array([H.fetch_slot(H._slot[d], 16 + i) for i in range(len(H.params))])


@pytest.mark.parametrize('prob_model', [False, True])
def test_mean_and_comoments_equal_the_replay_bit_for_bit(prob_model):
    from parasitoids_amd.predictive import ParamMoments, SensitivityMaps, SpreadSummary
    pm = _pop_model(prob_model=prob_model)
    T = _thetas()
    sets = [['mu_r'], THREE, None]                         # 1, 3 and 15 parameters
    W = float(sum(WEIGHTS))
    with contextlib.ExitStack() as stack:
        S = stack.enter_context(SpreadSummary(pm, DAYS))
        Hs = [stack.enter_context(SensitivityMaps(pm, p, DAYS)) for p in sets]
        assert [len(H.params) for H in Hs] == [1, 3, 15]
        assert Hs[2].nbytes == 6 * ((N * N + 63) // 64 * 64) * (18 * 8 + 1)
        mom = [ParamMoments(H.params) for H in Hs]
        state = [sens_ref.new_state((6, N, N), len(H.params)) for H in Hs]
        for mem, t, w in zip(MEMBERS, T, WEIGHTS):
            _evaluate(pm, mem)
            S.add(w)
            for H in Hs:
                H.add(t, w)
            f = _fields(pm)
            for H, m, st in zip(Hs, mom, state):
                sens_ref.add(st, f, m.update(t[_cols(H.params)], w), w)
        if prob_model:      # the device delta is in: every kept entry carries the renormalisation
            assert any(pm.stats[d].delta != 0.0 for d in range(5))
        for H, m, st in zip(Hs, mom, state):
            assert H.total_weight == W and H.members == 5
            assert np.array_equal(H.moments.C, m.C) and np.array_equal(H.moments.m, m.m)
            for d in DAYS:
                mean = H.mean(d)
                assert np.array_equal(mean, st['mean'][d]), (len(H.params), d)
                assert np.array_equal(mean, S.mean(d)) and np.array_equal(H.variance(d), S.variance(d))
                cov = _cov(H, d)
                assert np.array_equal(cov, st['C'][:, d] / W), (len(H.params), d)
            assert np.abs(_cov(H, 5)).max() > 0
    pm.close()


def test_covariance_maps_match_a_numpy_two_pass():
    from parasitoids_amd.predictive import SensitivityMaps
    pm = _pop_model()
    T = _thetas()
    fields = []
    with SensitivityMaps(pm, None, DAYS) as H:
        for mem, t, w in zip(MEMBERS, T, WEIGHTS):
            _evaluate(pm, mem)
            H.add(t, w)
            fields.append(_fields(pm))
        cols = _cols(None)
        mean, var, cov, tcov = sens_ref.two_pass(fields, T[:, cols], WEIGHTS)
        scale, sd = _scale_sd(mean, T, WEIGHTS, cols)
        for i, d in enumerate(DAYS):
            np.testing.assert_allclose(H.mean(d), mean[i], rtol=1e-12, atol=1e-15 * scale)
            np.testing.assert_allclose(H.variance(d), var[i], rtol=1e-12, atol=1e-15 * scale ** 2)
            got = _cov(H, d)
            for k, name in enumerate(H.params):
                print('day %d %-9s max |cov - two-pass| = %.3g of scale sd = %.3g'
                      % (d, name, np.abs(got[k] - cov[k, i]).max(), scale * sd[k]))
                np.testing.assert_allclose(got[k], cov[k, i], rtol=1e-12, atol=1e-15 * scale * sd[k])
                assert np.array_equal(got[k], H.covariance(d, name))
        sdm = np.sqrt(np.diag(tcov))
        np.testing.assert_allclose(H.moments.cov(), tcov, rtol=1e-12, atol=1e-15 * np.outer(sdm, sdm).max())
        # eleven of the fifteen parameters never move: their maps are exactly 0
        const = H.moments.constant()
        assert const.sum() == 11 and not got[const].any() and np.abs(got[~const]).max(axis=(1, 2)).min() > 0
    pm.close()


def test_weight_three_equals_three_unit_adds():
    from parasitoids_amd.predictive import SensitivityMaps
    pm = _pop_model()
    T = _thetas()
    with SensitivityMaps(pm, THREE) as A, SensitivityMaps(pm, THREE) as B:
        for mem, t, (wa, nb) in zip(MEMBERS[:3], T, ((1, 1), (3, 3), (2, 2))):
            _evaluate(pm, mem)
            A.add(t, wa)
            for _ in range(nb):
                B.add(t, 1)
        assert A.total_weight == B.total_weight == 6 and B.members == 6 and A.members == 3
        scale, sd = _scale_sd(A.mean(5), T[:3], (1, 3, 2), _cols(THREE))
        for d in A.days:
            ma = A.mean(d)
            np.testing.assert_allclose(ma, B.mean(d), rtol=1e-13, atol=1e-16 * np.abs(ma).max())
            np.testing.assert_allclose(A.variance(d), B.variance(d), rtol=1e-13,
                                       atol=1e-13 * 1e-3 * np.abs(ma).max() ** 2)
            for k, name in enumerate(THREE):
                np.testing.assert_allclose(A.covariance(d, name), B.covariance(d, name), rtol=1e-13,
                                           atol=1e-13 * 1e-3 * np.abs(ma).max() * sd[k])
    pm.close()


def test_merge_equals_one_handle_over_all_members():
    from parasitoids_amd.predictive import SensitivityMaps
    pm = _pop_model()
    T = _thetas()
    with SensitivityMaps(pm, THREE) as all_, SensitivityMaps(pm, THREE) as a, SensitivityMaps(pm, THREE) as b:
        for i, (mem, t, w) in enumerate(zip(MEMBERS, T, WEIGHTS)):
            _evaluate(pm, mem)
            all_.add(t, w)
            (a if i < 2 else b).add(t, w)
        a.merge(b)
        assert a.total_weight == all_.total_weight and a.members == all_.members == 5
        _scale, sd = _scale_sd(all_.mean(5), T, WEIGHTS, _cols(THREE))
        for d in a.days:
            m = all_.mean(d)
            np.testing.assert_allclose(a.mean(d), m, rtol=1e-12, atol=1e-15 * np.abs(m).max())
            np.testing.assert_allclose(a.variance(d), all_.variance(d), rtol=1e-12, atol=1e-15 * np.abs(m).max() ** 2)
            for k, name in enumerate(THREE):
                np.testing.assert_allclose(a.covariance(d, name), all_.covariance(d, name), rtol=1e-12,
                                           atol=1e-15 * np.abs(m).max() * sd[k])
        # merging into an empty handle is a copy, bit for bit
        with SensitivityMaps(pm, THREE) as e:
            e.merge(all_)
            assert e.total_weight == all_.total_weight and e.members == 5
            for d in e.days:
                assert np.array_equal(e.mean(d), all_.mean(d)) and np.array_equal(e.variance(d), all_.variance(d))
                assert np.array_equal(_cov(e, d), _cov(all_, d))
            assert np.array_equal(e.moments.C, all_.moments.C)
            keep = _cov(all_, 3)                           # and an empty source changes nothing
            with SensitivityMaps(pm, THREE) as none:
                all_.merge(none)
            assert np.array_equal(_cov(all_, 3), keep) and all_.members == 5
        with SensitivityMaps(pm, ['sig_x', 'mu_r']) as other:
            with pytest.raises(ValueError, match='different days or parameters'):
                a.merge(other)
    pm.close()


def test_properties_of_the_correlation_maps():
    from parasitoids_amd.predictive import SensitivityMaps
    pm = _pop_model()
    T = _thetas()
    names = _names()
    params = ['sig_x', 'sig_y', 'corr_p', 'mu_r']
    ix, iy, ic, im = (names.index(p) for p in params)
    fields = []
    cell = None
    with SensitivityMaps(pm, params) as H:
        for mem, t, w in zip(MEMBERS, T, WEIGHTS):
            _evaluate(pm, mem)
            f = _fields(pm)
            fields.append(f)
            if cell is None:
                cell = np.unravel_index(np.argmax(f[3]), f[3].shape)
            t = t.copy()
            t[iy] = t[ix]                                  # a duplicated parameter
            t[ic] = 0.5                                    # a constant one
            t[im] = f[3][cell]                             # and one that IS the population of a plume cell
            H.add(t, w)
        assert f[3][cell] > 1.0
        r = H.correlation(3, 'mu_r')
        assert abs(r[cell] - 1.0) <= 1e-12, r[cell]
        dead = ~(np.array(fields) != 0).any(axis=0)        # [day, N, N]: every member is 0 there
        assert all(dead[d].any() for d in DAYS) and dead[0].sum() > dead[5].sum()
        for d in DAYS:
            assert np.array_equal(H.covariance(d, 'sig_x'), H.covariance(d, 'sig_y'))
            assert np.array_equal(H.correlation(d, 'sig_x'), H.correlation(d, 'sig_y'))
            assert not H.covariance(d, 'corr_p').any() and not H.correlation(d, 'corr_p').any()
            for p in params:
                c = H.correlation(d, p)
                assert np.all(np.isfinite(c)) and np.abs(c).max() <= 1.0 + 1e-9
                assert not c[dead[d]].any() and not H.covariance(d, p)[dead[d]].any()
            assert not H.mean(d)[dead[d]].any() and not H.variance(d)[dead[d]].any()
        assert H.moments.constant().tolist() == [False, False, True, False]
        rank, dropped = H.finalize()
        assert rank == 2 and dropped.size == 1             # the constant one is not in the count, the copy is dropped
        assert set(np.unique(H.dominant(3))) <= {-1, 0, 3}     # never the copy (strict >), never the constant
        assert H.explained(3)[cell] >= 1.0 - 1e-9          # the cell's own value explains it
    pm.close()


def test_finalize_equals_its_replay_bit_for_bit():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import SensitivityMaps
    pm = _pop_model()
    T = _thetas()
    with SensitivityMaps(pm, THREE) as H:
        out = np.empty((N, N))
        for mem, t, w in zip(MEMBERS, T, WEIGHTS):
            _evaluate(pm, mem)
            H.add(t, w)
        for what in (2, 3):
            rc = H._lib.ps_sens_fetch(H._h, 0, what, L.p_f64(out))
            assert rc == L.PS_ERR_STATE and b'not finalized' in H._lib.ps_last_error()
        rank, dropped = H.finalize()
        assert rank == 3 and dropped.size == 0 and H.F.shape == (3, 3)
        for d in DAYS:
            var = H.variance(d)
            expl, dom = sens_ref.finalize(_cov(H, d), var, H.F, H.isd)
            got, gd = H.explained(d), H.dominant(d)
            assert gd.dtype == np.int8
            assert np.array_equal(got, expl), (d, np.abs(got - expl).max())
            assert np.array_equal(gd, dom), d
            assert got.min() >= 0.0 and got.max() <= 1.0 + 1e-9
            assert np.array_equal(gd == -1, var == 0.0) and not got[var == 0.0].any()
        assert H.explained(5).max() > 0.5 and H.dominant(5).max() >= 0
        # five members and three parameters leave one degree of freedom: not everything is explained
        assert H.explained(5)[H.variance(5) > 0].min() < 0.999
        _evaluate(pm, MEMBERS[1])
        H.add(T[1], 1)                                     # one more add: the result is stale
        for what in (2, 3):
            with pytest.raises(L.HipError) as err:
                H.fetch_slot(0, what)
            assert err.value.code == L.PS_ERR_STATE
        H.finalize()
        H.explained(0)
        with SensitivityMaps(pm, THREE) as other:
            other.add(T[0], 1)
            H.merge(other)                                 # and so it is after a merge
            with pytest.raises(L.HipError) as err:
                H.dominant(0)
            assert err.value.code == L.PS_ERR_STATE
        # too few members: refused on the host, the correlations stay available
        H.reset()
        for mem, t in zip(MEMBERS[:4], T):
            _evaluate(pm, mem)
            H.add(t, 2)
        with pytest.raises(ValueError, match='4 members for 3 independent'):
            H.finalize()
        assert np.abs(H.correlation(5, 'mu_r')).max() > 0.5
    pm.close()


def test_projections_and_release_plans_as_sources():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import (ParamMoments, Projection, ReleaseSites, SensitivityMaps, exposure_weights,
                                            lagged_models)
    pm = _pop_model()
    T = _thetas()
    res = 10000.0 / 128
    late = lagged_models(pm, [0, 2])
    plan = [(0.0, 0.0, 0.6, 0), (13 * res, 6 * res, 0.4, 2)]      # two sites, the second released two days later
    W = exposure_weights([0, 1, 2], [0, 1, 2])
    with Projection(pm, W, [0, 1, 2]) as P, ReleaseSites(pm, plan, [0, 2, 3, 5], late) as RS, \
            SensitivityMaps.for_projection(P, THREE) as HP_, SensitivityMaps.for_projection(RS, THREE) as HS:
        lib = HP_._lib
        e = L.f64([0.0, 0.0, 0.0])
        assert lib.ps_sens_add_project(HP_._h, P._h, 3, L.p_f64(e), 1) == L.PS_ERR_STATE     # nothing applied yet
        assert lib.ps_sens_add_sites(HS._h, RS._h, 3, L.p_f64(e), 1) == L.PS_ERR_STATE
        mom = ParamMoments(THREE)
        sp, ss = sens_ref.new_state((3, N, N), 3), sens_ref.new_state((4, N, N), 3)
        for mem, t, w in zip(MEMBERS, T, WEIGHTS):
            _evaluate(pm, mem)
            _evaluate(late[2], mem, ndays=4)
            P.apply()
            RS.apply()
            HP_.add(t, w)
            HS.add(t, w)
            ev = mom.update(t[_cols(THREE)], w)
            sens_ref.add(sp, np.array([P.field(k) for k in range(3)]), ev, w)
            sens_ref.add(ss, np.array([RS.field(k) for k in range(4)]), ev, w)
        Wt = float(sum(WEIGHTS))
        for H, st, n in ((HP_, sp, 3), (HS, ss, 4)):
            assert H.members == 5 and H.days == list(range(n))
            for k in range(n):
                assert np.array_equal(H.mean(k), st['mean'][k])
                assert np.array_equal(_cov(H, k), st['C'][:, k] / Wt)
            assert np.abs(_cov(H, n - 1)).max() > 0
        # the exposure up to day 2 is a sum over days: its covariance is the sum of the days' covariances
        with SensitivityMaps(pm, THREE, [0, 1, 2]) as D:
            for mem, t, w in zip(MEMBERS, T, WEIGHTS):
                _evaluate(pm, mem)
                D.add(t, w)
            tot = sum(_cov(D, d) for d in (0, 1, 2))
            np.testing.assert_allclose(_cov(HP_, 2), tot, rtol=1e-10, atol=1e-12 * np.abs(tot).max())
        # a read while a pass over the plan's groups is open is refused, and adds nowhere
        calls = RS._calls()
        L.check(lib.ps_sites_apply(RS._h, *calls[0]))
        with pytest.raises(L.HipError) as err:
            HS.add(T[0], 1)
        assert err.value.code == L.PS_ERR_STATE and HS.members == 5 and HS.moments.members == 5
        L.check(lib.ps_sites_apply(RS._h, *calls[1]))
        HS.add(T[0], 1)
        assert HS.members == 6 and HS.moments.W == sum(WEIGHTS) + 1
    for m in (pm, late[2]):
        m.close()


def test_the_other_accumulators_are_untouched():
    """SpreadSummary, SpreadHistogram and ArrivalMaps give the same bits with and without a SensitivityMaps
    alongside (fresh models: an auto-mode model routes days by what it has seen before)"""
    from parasitoids_amd.predictive import ArrivalMaps, SensitivityMaps, SpreadHistogram, SpreadSummary
    T = _thetas()
    days = [0, 2, 5]

    def run(with_sens):
        pm = _pop_model()
        with SpreadSummary(pm, days, (1.0, 50.0)) as S, SpreadHistogram(pm, days, (1e-8, 1e6, 2)) as Hh, \
                ArrivalMaps(pm, [1.0, 10.0], days) as A, contextlib.ExitStack() as stack:
            X = stack.enter_context(SensitivityMaps(pm, THREE, days)) if with_sens else None
            for mem, t, w in zip(MEMBERS, T, WEIGHTS):
                _evaluate(pm, mem)
                S.add(w)
                if X is not None:
                    X.add(t, w)
                Hh.add(w)
                A.add(w)
            if X is not None:
                X.finalize()
            out = [S.mean(d) for d in days] + [S.variance(d) for d in days]
            out += [S.exceedance(d, k) for d in days for k in (0, 1)] + [Hh.counts(d) for d in days]
            out += [A.counts(k, d) for k in (0, 1) for d in days + [None]] + [A.reached(0)[0]]
        pm.close()
        return out
    a, b = run(False), run(True)
    assert len(a) == len(b) == 24 and all(np.array_equal(x, y) for x, y in zip(a, b))


def _csr(f, key):
    return sparse.csr_matrix((f[key + '_data'], f[key + '_ind'], f[key + '_indptr']), shape=(N, N)).toarray()


def test_end_to_end_is_reproducible_and_saves(tmp_path):
    from parasitoids_amd.predictive import posterior_predictive
    days = [0, 2, 5]
    tr = _member_trace(MEMBERS, WEIGHTS)

    def run():
        pm = _pop_model()
        res = posterior_predictive(pm, tr, days=days, thresholds=(1.0,), sensitivity=THREE, exposure=[2, 5])
        return pm, res
    pa, a = run()
    pb, b = run()
    X, Y = a.sensitivity, b.sensitivity
    assert X.params == THREE and X.members == 5 and X.total_weight == 8 and X.days == days
    for d in days:
        assert np.array_equal(X.mean(d), Y.mean(d)) and np.array_equal(X.mean(d), a.summary.mean(d))
        assert np.array_equal(X.variance(d), a.summary.variance(d))
        assert np.array_equal(_cov(X, d), _cov(Y, d))
    ex = a.exposure.sensitivity
    assert ex is not None and ex.members == 5 and np.array_equal(ex.mean(1), a.exposure.summary.mean(1))
    assert np.array_equal(_cov(ex, 1), _cov(b.exposure.sensitivity, 1))
    npz, js = a.save(str(tmp_path / 'out' / 'pp'), {'site': 'kalbar'})      # finalizes the maps it writes
    Y.finalize()
    assert np.array_equal(X.explained(5), Y.explained(5)) and np.array_equal(X.dominant(5), Y.dominant(5))
    with np.load(str(tmp_path / 'out' / 'pp_sens.npz')) as f:
        assert list(f['days']) == [pa.days[d] for d in days]
        for d in days:
            label = str(pa.days[d])
            r2, dom = X.explained(d), X.dominant(d)
            assert np.array_equal(_csr(f, label + '_r2'), np.where(r2 >= 1e-8, r2, 0.0))
            assert f[label + '_dom'].dtype == np.int8 and np.array_equal(f[label + '_dom'], dom)
            for name in THREE:
                c = X.correlation(d, name)
                assert np.array_equal(_csr(f, '%s_corr_%s' % (label, name)), np.where(np.abs(c) >= 1e-8, c, 0.0))
        assert _csr(f, str(pa.days[5]) + '_corr_sig_x').min() < 0          # a signed map
    with np.load(str(tmp_path / 'out' / 'pp_exposure_sens.npz')) as f:
        assert list(f['days']) == [2, 5] and '5_r2_data' in f and '2_corr_mu_r_data' in f and '2_dom' in f
    meta = json.load(open(js))['predictive']
    blk = meta['sensitivity']
    assert blk['params'] == THREE and blk['members'] == 5 and blk['total_weight'] == 8 and blk['finalized'] is True
    assert blk['rank'] == 3 and blk['dropped_eigenvalues'] == [] and 'reason' not in blk
    T = tr[0][:, _cols(THREE)]
    np.testing.assert_allclose(blk['mean'], T.mean(0), rtol=1e-13)
    np.testing.assert_allclose(blk['sd'], T.std(0), rtol=1e-12)
    np.testing.assert_allclose(blk['correlation'], np.corrcoef(T.T), rtol=1e-10, atol=1e-12)
    assert meta['exposure']['sensitivity']['params'] == THREE and meta['exposure']['sensitivity']['finalized'] is True
    for r in (a, b):
        r.summary.close()
        r.sensitivity.close()
        r.exposure.close()
    for p in (pa, pb):
        p.close()


def test_parallel_chains_equal_sequential_and_too_few_members(tmp_path):
    from parasitoids_amd.predictive import posterior_predictive
    days = [0, 2, 5]
    c1 = _member_trace(MEMBERS[:3], [2, 1, 3])
    c2 = _member_trace(MEMBERS[2:], [1, 4, 2])
    kw = dict(days=days, thresholds=(1.0,), sensitivity=THREE)
    pa, pb = _pop_model(), _pop_model()
    par = posterior_predictive([pa, pb], [c1, c2], **kw)
    pc, pd = _pop_model(), _pop_model()
    s1 = posterior_predictive(pc, c1, **kw)
    s2 = posterior_predictive(pd, c2, **kw)
    # three members cannot carry two independent parameters: the correlations are saved, with the reason
    npz, js = s1.save(str(tmp_path / 'few'))
    blk = json.load(open(js))['predictive']['sensitivity']
    assert blk['finalized'] is False and '3 members for 2 independent' in blk['reason'] and blk['rank'] == 2
    with np.load(str(tmp_path / 'few_sens.npz')) as f:
        label = str(pc.days[5])
        assert label + '_corr_mu_r_data' in f and label + '_r2_data' not in f and label + '_dom' not in f
        c = s1.sensitivity.correlation(5, 'mu_r')
        assert np.array_equal(_csr(f, label + '_corr_mu_r'), np.where(np.abs(c) >= 1e-8, c, 0.0))
    s1.sensitivity.merge(s2.sensitivity)
    X, Y = par.sensitivity, s1.sensitivity
    assert X.members == Y.members == 6 and X.total_weight == Y.total_weight == 13
    assert np.array_equal(X.moments.C, Y.moments.C) and np.array_equal(X.moments.m, Y.moments.m)
    X.finalize()
    Y.finalize()
    for d in days:
        assert np.array_equal(X.mean(d), Y.mean(d)) and np.array_equal(X.variance(d), Y.variance(d))
        assert np.array_equal(_cov(X, d), _cov(Y, d))
        assert np.array_equal(X.explained(d), Y.explained(d)) and np.array_equal(X.dominant(d), Y.dominant(d))
    for r in (par, s1, s2):
        r.summary.close()
        r.sensitivity.close()
    for p in (pa, pb, pc, pd):
        p.close()


def test_c_abi_refusals():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import NEGVAL, Projection, SensitivityMaps, _day_scales, exposure_weights
    pm = _pop_model()
    other = _pop_model(R=64, ndays=3)
    _evaluate(pm, MEMBERS[0])
    _evaluate(other, MEMBERS[0])
    lib = L.load()
    T = _thetas()

    def refused(rc, code, *words):
        msg = lib.ps_last_error()
        assert rc == code, (rc, msg)
        for w in words:
            assert w in msg, msg

    # create: the limits, and the whole block against the free memory before anything is allocated
    h = L._VP()
    for nslot, nparam in ((1, 0), (1, 17), (0, 3)):
        refused(lib.ps_sens_create(0, N, nslot, nparam, C.byref(h)), L.PS_ERR_BAD_ARG, b'sens_create', b'parameters')
    refused(lib.ps_sens_create(0, 801, 200000, 16, C.byref(h)), L.PS_ERR_OOM, b'sens_create', b'GB free')
    assert not h
    with SensitivityMaps(pm, THREE, [0, 1, 2]) as H, SensitivityMaps(pm, THREE, [0, 1]) as H2, \
            SensitivityMaps(pm, ['mu_r'], [0, 1, 2]) as H1, SensitivityMaps(other, THREE, [0, 1, 2]) as Ho:
        out = np.empty((N, N))
        refused(lib.ps_sens_fetch(H._h, 0, 0, L.p_f64(out)), L.PS_ERR_STATE, b'nothing accumulated')
        F, isd = L.f64(np.eye(3)), L.f64([1.0, 1.0, 1.0])
        refused(lib.ps_sens_finalize(H._h, 3, 3, L.p_f64(F), L.p_f64(isd)), L.PS_ERR_STATE, b'nothing accumulated')
        stat, post = _day_scales(pm, H.days)
        e = L.f64([0.1, -0.2, 0.3])

        def add(h=H, solver=pm, nslot=3, nparam=3, e=e, w=1):
            return lib.ps_sens_add(h._h, solver.solver._h, nslot, L.p_i32(H._kind), L.p_i32(H._idx), L.p_f64(stat),
                                   L.p_f64(post), L.p_i32(H._delta), NEGVAL, nparam, L.p_f64(e), w)
        refused(add(nparam=2), L.PS_ERR_BAD_ARG, b'2 parameters given', b'has 3')
        refused(add(nslot=2), L.PS_ERR_BAD_ARG, b'2 slots given', b'has 3')
        refused(add(w=0), L.PS_ERR_BAD_ARG, b'weight must be >= 1')
        for bad in (np.nan, np.inf, -np.inf):
            refused(add(e=L.f64([0.1, bad, 0.3])), L.PS_ERR_BAD_ARG, b'e[1] is not finite')
        refused(add(solver=other), L.PS_ERR_BAD_ARG, b'solver domain 129', b'handle domain 257')
        assert H.members == 0 and H.total_weight == 0               # none of them enqueued anything
        assert add() == L.PS_OK
        refused(add(w=0xffffffff), L.PS_ERR_BAD_ARG, b'total weight 4294967296', b'2^32')
        assert add(w=0xfffffffe) == L.PS_OK and H.total_weight == 2.0 ** 32 - 1
        refused(add(), L.PS_ERR_BAD_ARG, b'2^32')
        L.check(lib.ps_sens_reset(H._h))
        assert add() == L.PS_OK
        # merge
        d3, d1 = L.f64([0.0, 0.0, 0.0]), L.f64([0.0])
        refused(lib.ps_sens_merge(H._h, H._h, 3, L.p_f64(d3)), L.PS_ERR_BAD_ARG, b'same handle')
        refused(lib.ps_sens_merge(H._h, H1._h, 3, L.p_f64(d3)), L.PS_ERR_BAD_ARG, b'3 parameters given', b'src 1')
        refused(lib.ps_sens_merge(H._h, H1._h, 1, L.p_f64(d1)), L.PS_ERR_BAD_ARG, b'1 parameters given', b'dst has 3')
        refused(lib.ps_sens_merge(H._h, H2._h, 3, L.p_f64(d3)), L.PS_ERR_BAD_ARG, b'dst has 3 slots, src 2')
        refused(lib.ps_sens_merge(H._h, Ho._h, 3, L.p_f64(d3)), L.PS_ERR_BAD_ARG, b'dst domain 257, src domain 129')
        with SensitivityMaps(pm, THREE, [0, 1, 2]) as Hb:
            refused(lib.ps_sens_merge(H._h, Hb._h, 3, L.p_f64(L.f64([0.0, np.nan, 0.0]))), L.PS_ERR_BAD_ARG,
                    b'dtheta[1] is not finite')
        # finalize and fetch
        refused(lib.ps_sens_finalize(H._h, 2, 2, L.p_f64(F), L.p_f64(isd)), L.PS_ERR_BAD_ARG, b'factor 2 x 2', b'3 param')
        refused(lib.ps_sens_finalize(H._h, 3, 17, L.p_f64(F), L.p_f64(isd)), L.PS_ERR_BAD_ARG, b'rank 1..16')
        Fb = F.copy()
        Fb[0, 1] = np.inf
        refused(lib.ps_sens_finalize(H._h, 3, 3, L.p_f64(Fb), L.p_f64(isd)), L.PS_ERR_BAD_ARG, b'F[0][1] is not finite')
        refused(lib.ps_sens_finalize(H._h, 3, 3, L.p_f64(F), L.p_f64(L.f64([1.0, 1.0, np.nan]))), L.PS_ERR_BAD_ARG,
                b'isd[2] is not finite')
        for what in (2, 3):
            refused(lib.ps_sens_fetch(H._h, 0, what, L.p_f64(out)), L.PS_ERR_STATE, b'not finalized')
        refused(lib.ps_sens_fetch(H._h, 3, 0, L.p_f64(out)), L.PS_ERR_BAD_ARG, b'slot 3 of 3')
        for what in (4, 15, 19, -1):
            refused(lib.ps_sens_fetch(H._h, 0, what, L.p_f64(out)), L.PS_ERR_BAD_ARG, b'quantity')
        assert lib.ps_sens_finalize(H._h, 3, 3, L.p_f64(F), L.p_f64(isd)) == L.PS_OK
        assert lib.ps_sens_fetch(H._h, 0, 3, L.p_f64(out)) == L.PS_OK and set(np.unique(out)) <= {-1.0, 0.0, 1.0, 2.0}
        # the other sources: a projection of another shape, and one that has no fields yet
        with Projection(pm, exposure_weights([0, 1], [0, 1]), [0, 1]) as P2, \
                Projection(pm, exposure_weights([0, 1, 2], [0, 1, 2]), [0, 1, 2]) as P3:
            refused(lib.ps_sens_add_project(H._h, P3._h, 3, L.p_f64(e), 1), L.PS_ERR_STATE)
            P2.apply()
            P3.apply()
            refused(lib.ps_sens_add_project(H._h, P2._h, 3, L.p_f64(e), 1), L.PS_ERR_BAD_ARG,
                    b'sens_add_project: the projection has 2 outputs, the handle 3 slots')
            assert lib.ps_last_error() == b'sens_add_project: the projection has 2 outputs, the handle 3 slots'
            refused(lib.ps_sens_add_project(H._h, P3._h, 2, L.p_f64(e), 1), L.PS_ERR_BAD_ARG, b'sens_add_project',
                    b'2 parameters given')
            refused(lib.ps_sens_add_project(H._h, P3._h, 3, L.p_f64(e), 0), L.PS_ERR_BAD_ARG, b'weight must be >= 1')
            refused(lib.ps_sens_add_project(Ho._h, P3._h, 3, L.p_f64(e), 1), L.PS_ERR_BAD_ARG,
                    b'sens_add_project: projection domain 257, handle domain 129')
            assert lib.ps_last_error() == b'sens_add_project: projection domain 257, handle domain 129'
            assert lib.ps_sens_add_project(H._h, P3._h, 3, L.p_f64(e), 1) == L.PS_OK and H.members == 2
        # the wrapper: a theta of the wrong length, a model that has not run far enough, names
        with pytest.raises(ValueError, match='theta has 3 entries'):
            H.add([1.0, 2.0, 3.0])
        with pytest.raises(ValueError, match='unknown sensitivity'):
            SensitivityMaps(pm, ['nope'])
        with pytest.raises(ValueError, match='is not among'):
            H.covariance(0, 'lam')
        with pytest.raises(ValueError, match='day 4 is not in'):
            H.mean(4)
        short = _pop_model(ndays=6)
        _evaluate(short, MEMBERS[0], ndays=2)
        with SensitivityMaps(short, THREE, [0, 1, 2]) as Hs:
            with pytest.raises(ValueError, match='sensitivity maps needs day 2'):
                Hs.add(T[0], 1)
            assert Hs.moments.members == 0
        short.close()
    refused(lib.ps_sens_reset(None), L.PS_ERR_BAD_ARG, b'null handle')
    refused(lib.ps_sens_info(None, None, None), L.PS_ERR_BAD_ARG, b'null handle')
    pm.close()
    other.close()
