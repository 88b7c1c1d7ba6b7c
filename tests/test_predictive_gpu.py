"""GPU tests of the posterior predictive spread (ps_summary_*, parasitoids_amd/predictive.py): the
device accumulator against a numpy weighted two-pass over `PopModel.population(d)`, weights,
merging, solver switches, bitwise reproducibility, the end-to-end chain reader, the oracle and the
saved result file.  Kalbar wind, R = 128, 6 days unless stated."""
import os
import warnings

import numpy as np
import pytest
from scipy import sparse

from helpers import HP, DP, DLP, MU_R, NPER

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.abspath(__file__))
MEMBERS = [(DP, MU_R), ((160.0, 150.0, 0.2), 1.1), ((185.0, 140.0, 0.3), 1.25), ((171.82, 160.0, 0.1), 1.0),
           ((150.0, 135.0, 0.28), 1.15)]
WEIGHTS = [1, 3, 1, 2, 1]


def _wind():
    from parasitoids_amd import ParasitoidModel as PM
    return PM.get_wind_data(os.path.join(ROOT, 'golden', 'data', 'kalbar'), 30, '00:00')


def _pop_model(R=128, ndays=6, **kw):
    from parasitoids_amd.pop_model import PopModel
    wd, days = _wind()
    return PopModel(wd, days[:ndays], domain_info=(10000.0, R), r_number=130000, **kw)


def _evaluate(pm, member):
    dp, mu = member
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        pm.evaluate(HP, dp, DLP, mu, NPER, want_stats=False)


def _fields(pm, days):
    return [pm.population(d).toarray() for d in days]


def _two_pass(fields, weights, thresholds):
    """weighted mean, variance (M2 / W) and exceedance counts from the dense fields [member][day]"""
    w = np.asarray(weights, dtype=np.float64)
    X = np.asarray(fields)                       # [member, day, N, N]
    W = w.sum()
    mean = np.tensordot(w, X, axes=1) / W
    var = np.tensordot(w, (X - mean[None]) ** 2, axes=1) / W
    counts = [np.tensordot(np.asarray(weights, dtype=np.int64), (X >= t).astype(np.int64), axes=1) for t in thresholds]
    return mean, var, counts


def _check(S, days, ref, thresholds, rtol=1e-12):
    mean, var, counts = ref
    W = S.total_weight
    for i, d in enumerate(days):
        m = S.mean(d)
        scale = np.abs(mean[i]).max()
        np.testing.assert_allclose(m, mean[i], rtol=rtol, atol=rtol * 1e-3 * scale)
        np.testing.assert_allclose(S.variance(d), var[i], rtol=rtol, atol=rtol * 1e-3 * scale ** 2)
        for k in range(len(thresholds)):
            c = S.exceedance(d, k) * W
            assert np.array_equal(np.rint(c).astype(np.int64), counts[k][i]), (d, k)


@pytest.mark.parametrize('prob_model', [False, True])
def test_weighted_moments_match_a_numpy_two_pass(prob_model):
    from parasitoids_amd.predictive import SpreadSummary
    pm = _pop_model(prob_model=prob_model)
    thr = (1e-6, 1e-3) if prob_model else (1.0, 100.0)
    days = list(range(6))
    fields = []
    with SpreadSummary(pm, days, thr) as S:
        for mem, w in zip(MEMBERS, WEIGHTS):
            _evaluate(pm, mem)
            S.add(w)
            fields.append(_fields(pm, days))
        assert S.total_weight == sum(WEIGHTS) and S.members == len(MEMBERS)
        ref = _two_pass(fields, WEIGHTS, thr)
        _check(S, days, ref, thr)
        if prob_model:      # the device delta is in: every kept entry carries the renormalisation
            assert any(pm.stats[d].delta != 0.0 for d in range(5))
        assert np.all(S.variance(3) >= 0) and S.sd(3).max() > 0
    pm.close()


def test_weight_three_equals_three_unit_adds():
    from parasitoids_amd.predictive import SpreadSummary
    pm = _pop_model()
    thr = (1.0, 100.0)
    with SpreadSummary(pm, None, thr) as A, SpreadSummary(pm, None, thr) as B:
        for mem, (wa, nb) in zip(MEMBERS[:3], ((1, 1), (3, 3), (2, 2))):
            _evaluate(pm, mem)
            A.add(wa)
            for _ in range(nb):
                B.add(1)
        assert A.total_weight == B.total_weight == 6 and B.members == 6
        for d in A.days:
            ma, mb = A.mean(d), B.mean(d)
            np.testing.assert_allclose(ma, mb, rtol=1e-13, atol=1e-16 * np.abs(ma).max())
            va, vb = A.variance(d), B.variance(d)
            np.testing.assert_allclose(va, vb, rtol=1e-13, atol=1e-13 * 1e-3 * np.abs(ma).max() ** 2)
            for k in range(2):
                assert np.array_equal(A.exceedance(d, k), B.exceedance(d, k))
    pm.close()


def test_merge_equals_one_summary_over_all_members():
    from parasitoids_amd.predictive import SpreadSummary
    pm = _pop_model()
    thr = (1.0,)
    with SpreadSummary(pm, None, thr) as all_, SpreadSummary(pm, None, thr) as a, \
            SpreadSummary(pm, None, thr) as b:
        for i, (mem, w) in enumerate(zip(MEMBERS, WEIGHTS)):
            _evaluate(pm, mem)
            all_.add(w)
            (a if i < 2 else b).add(w)
        a.merge(b)
        assert a.total_weight == all_.total_weight and a.members == all_.members
        for d in a.days:
            m = all_.mean(d)
            np.testing.assert_allclose(a.mean(d), m, rtol=1e-12, atol=1e-15 * np.abs(m).max())
            np.testing.assert_allclose(a.variance(d), all_.variance(d), rtol=1e-12,
                                       atol=1e-15 * np.abs(m).max() ** 2)
            assert np.array_equal(a.exceedance(d, 0), all_.exceedance(d, 0))
        # merging into an empty summary is a copy
        with SpreadSummary(pm, None, thr) as e:
            e.merge(all_)
            assert all(np.array_equal(e.mean(d), all_.mean(d)) for d in e.days)
    pm.close()


def test_members_on_different_cached_solvers_in_exact_mode():
    """the kernel extent moves with the diffusion parameters; in exact mode each extent has its own
    solver and stream, and successive adds from them are ordered by the summary's event"""
    from parasitoids_amd.predictive import SpreadSummary
    pm = _pop_model(mode='exact')
    mems = [((120.0, 100.0, 0.2), 1.0), ((260.0, 230.0, 0.25), 1.2), ((120.0, 100.0, 0.2), 1.05),
            ((200.0, 170.0, 0.1), 1.1)]
    w = [2, 1, 1, 3]
    days = list(range(6))
    fields, solvers = [], set()
    with SpreadSummary(pm, days, (10.0,)) as S:
        for mem, wi in zip(mems, w):
            _evaluate(pm, mem)
            solvers.add(id(pm.solver))
            S.add(wi)
        # the fields are read back only now: every add was enqueued behind the next evaluation
        for mem in mems:
            _evaluate(pm, mem)
            fields.append(_fields(pm, days))
        assert len(solvers) >= 2
        _check(S, days, _two_pass(fields, w, (10.0,)), (10.0,))
    pm.close()


def _member_trace(mems, repeats):
    from parasitoids_amd import mcmc
    t0 = np.array([m[2] for m in mcmc.MODEL_BLOCK])
    names = [m[0] for m in mcmc.MODEL_BLOCK]
    rows = []
    for (dp, mu), n in zip(mems, repeats):
        t = t0.copy()
        t[names.index('sig_x')], t[names.index('sig_y')], t[names.index('corr_p')] = dp[0], dp[1], (dp[2] + 1) / 2
        t[names.index('mu_r')] = mu
        rows += [t] * n
    return np.array(rows), names


def test_bitwise_reproducible_and_parallel_chains_equal_sequential():
    """the same members in the same order give the same bits; so do two chains in parallel (one
    PopModel and host thread each) and the chains one after another, merged in chain order.  Every
    path starts from fresh PopModels: an auto-mode model routes days by what it has seen before,
    which may move a field by rounding"""
    from parasitoids_amd.predictive import SpreadSummary, posterior_predictive
    days = [0, 2, 5]

    def run():
        pm = _pop_model()
        with SpreadSummary(pm, days, (1.0, 50.0)) as S:
            for mem, w in zip(MEMBERS, WEIGHTS):
                _evaluate(pm, mem)
                S.add(w)
            out = [S.mean(d) for d in days] + [S.variance(d) for d in days] + [S.exceedance(5, 1)]
        pm.close()
        return out
    a, b = run(), run()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    c1 = _member_trace(MEMBERS[:3], [2, 1, 3])
    c2 = _member_trace(MEMBERS[2:], [1, 4, 2])
    pa, pb = _pop_model(), _pop_model()
    par = posterior_predictive([pa, pb], [c1, c2], days=days, thresholds=(1.0,))
    pc, pd = _pop_model(), _pop_model()
    s1 = posterior_predictive(pc, c1, days=days, thresholds=(1.0,))
    s2 = posterior_predictive(pd, c2, days=days, thresholds=(1.0,))
    s1.summary.merge(s2.summary)
    assert par.evaluations == s1.evaluations + s2.evaluations == 6 and par.rows == 13
    assert par.summary.total_weight == s1.summary.total_weight == 13
    for d in days:
        assert np.array_equal(s1.summary.mean(d), par.summary.mean(d))
        assert np.array_equal(s1.summary.variance(d), par.summary.variance(d))
        assert np.array_equal(s1.summary.exceedance(d, 0), par.summary.exceedance(d, 0))
    for r in (par, s1, s2):
        r.summary.close()
    for p in (pa, pb, pc, pd):
        p.close()


def test_end_to_end_sampler_chain(tmp_path):
    from parasitoids_amd import mcmc
    from parasitoids_amd.predictive import observation_rates, posterior_predictive
    pm = _pop_model(ndays=18)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        li = mcmc.synthetic_locinfo(pm, 128, seed=9)
        cell_area = (10000.0 / 128) ** 2
        smp = mcmc.Sampler(pm, li, cell_area, seed=21)
        smp.run(10)
        smp.save(tmp_path / 'chain.npz')
        days = [0, 4, 9, 17]
        res = posterior_predictive(pm, str(tmp_path / 'chain.npz'), days=days, thresholds=(1.0,), locinfo=li,
                                   cell_area=cell_area, seed=3)
        assert res.rows == 10 and res.evaluations < res.rows and res.failed == 0
        # the explicit per-row loop: every row evaluated, weight 1
        tr = np.load(tmp_path / 'chain.npz')['trace']
        fields = []
        for row in tr:
            pm.evaluate(*mcmc.model_args(row[:15]), want_stats=False)
            fields.append(_fields(pm, days))
    _check(res.summary, days, _two_pass(fields, [1] * len(tr), (1.0,)), (1.0,))
    obs = res.observations
    for g in ('release', 'sentinel', 'grid'):
        assert np.all(np.isfinite(obs[g]['mean_rate'])) and 0.0 <= obs[g]['p_total'] <= 1.0
    # the observation predictive equals the per-row rates of the explicit loop
    rates = []
    for row in tr:
        pm.evaluate(*mcmc.model_args(row[:15]), want_stats=False)
        exp = mcmc.expected_observations(pm, li)
        rates.append(np.concatenate([np.ravel(r) for r in observation_rates(exp, li, row[15:18], row[19:])[0]]))
    np.testing.assert_allclose(obs['release']['mean_rate'], np.mean(rates, 0), rtol=1e-12, atol=0)
    res.summary.close()
    pm.close()


def test_mean_map_against_the_oracle():
    from oracle import calcsol as OC
    from oracle import model as OM
    from parasitoids_amd.predictive import SpreadSummary
    from helpers import recentre
    R, nd = 64, 6
    pm = _pop_model(R=R, ndays=nd, mode='exact')
    wd, days = _wind()
    mems = [MEMBERS[0], MEMBERS[2]]
    refs = []
    with SpreadSummary(pm) as S:
        for dp, mu in mems:
            _evaluate(pm, (dp, mu))
            S.add(1)
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)
                pmfs = [OM.prob_mass(d, wd, HP, dp, DLP, mu, NPER, 10000.0, R).tocoo() for d in days[:nd]]
            max_shape = np.max([p.shape for p in pmfs], axis=0)
            ref = OC.get_populations([recentre(pmfs[0], R).tocsr()], pmfs, days, nd, 2 * R + 1, max_shape, 1,
                                     130000, lambda day: 1.0)
            refs.append([r.toarray() for r in ref])
        for d in range(nd):
            np.testing.assert_allclose(S.mean(d), 0.5 * (refs[0][d] + refs[1][d]), rtol=1e-9, atol=1e-7)
    pm.close()


def test_saved_result_reloads_by_the_reference_loader_rule(tmp_path):
    from parasitoids_amd.predictive import posterior_predictive
    pm = _pop_model()
    tr = _member_trace(MEMBERS[:2], [2, 1])
    res = posterior_predictive(pm, tr, thresholds=(1.0, 100.0))
    npz, js = res.save(str(tmp_path / 'out' / 'pp'), {'site': 'kalbar', 'rad_res': 128})
    N = 257
    with np.load(npz) as f:        # Plot_Result.py:515-524
        labels = list(f['days'])
        assert labels == list(pm.days)
        for n, day in enumerate(labels):
            M = sparse.csr_matrix((f[str(day) + '_data'], f[str(day) + '_ind'], f[str(day) + '_indptr']), shape=(N, N))
            m = res.summary.mean(n)
            assert np.array_equal(M.toarray(), np.where(m >= 1e-8, m, 0.0))
            sd = sparse.csr_matrix((f[str(day) + '_sd_data'], f[str(day) + '_sd_ind'], f[str(day) + '_sd_indptr']),
                                   shape=(N, N))
            s = res.summary.sd(n)
            assert np.array_equal(sd.toarray(), np.where(s >= 1e-8, s, 0.0))
            assert str(day) + '_pexc1_data' in f
    import json
    meta = json.load(open(js))
    assert meta['site'] == 'kalbar' and meta['predictive']['thresholds'] == [1.0, 100.0]
    assert meta['predictive']['evaluations'] == 2 and meta['predictive']['rows'] == 3
    res.summary.close()
    pm.close()


def test_error_paths():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import SpreadSummary
    pm = _pop_model()
    other = _pop_model(R=64, ndays=3)
    _evaluate(pm, MEMBERS[0])
    _evaluate(other, MEMBERS[0])
    with SpreadSummary(pm, [0, 1, 2]) as S:
        with pytest.raises(L.HipError) as e:         # nothing accumulated yet
            S.mean(0)
        assert e.value.code == L.PS_ERR_STATE
        S.pm = other                                  # a solver of another domain
        with pytest.raises(L.HipError) as e:
            S.add(1)
        assert e.value.code == L.PS_ERR_BAD_ARG and S.members == 0
        S.pm = pm
        S.add(1)
        with pytest.raises(L.HipError) as e:
            S.fetch_slot(3, 0)
        assert e.value.code == L.PS_ERR_BAD_ARG
        with pytest.raises(L.HipError) as e:
            S.fetch_slot(0, 2)                        # no threshold
        assert e.value.code == L.PS_ERR_BAD_ARG
        S.reset()
        with pytest.raises(L.HipError) as e:
            S.variance(1)
        assert e.value.code == L.PS_ERR_STATE
    pm.close(); other.close()
