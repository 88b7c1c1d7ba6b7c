"""GPU tests of the projections over time (ps_project_*, predictive.Projection) and of the accumulators fed
from them (SpreadSummary.for_projection, SpreadHistogram.for_projection): the device fields bit for bit
against the numpy reference (project_ref.project of `PopModel.population(d)`), the reference's own emergence
numbers of the G9 fixture, the posterior of a sum against the sum of posteriors, histograms, add and merge
order, solver switches, the untouched day-based paths, the refusals, and posterior_predictive with
emergence= / exposure=.  Kalbar wind, R = 128, 6 days, the members and weights of test_arrival_gpu.py."""
import ctypes as C
import json
import os
import types
import warnings

import numpy as np
import pytest

from helpers import HP, DP, DLP, MU_R, NPER
from hist_ref import exact_quantile, weighted_counts
from project_ref import project

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.abspath(__file__))
MEMBERS = [(DP, MU_R), ((160.0, 150.0, 0.2), 1.1), ((185.0, 140.0, 0.3), 1.25), ((171.82, 160.0, 0.1), 1.0),
           ((150.0, 135.0, 0.28), 1.15)]
WEIGHTS = [1, 3, 1, 2, 1]
THR = [1.0, 10.0]
DAYS = list(range(6))
UPTO = [0, 2, 5]
# 9 outputs x 6 inputs: two output tiles.  Record 4 is used by no tile at all; the first tile (outputs
# 0..7) skips records 4 and 5, the second (output 8) reads record 5 alone.
HAND_W = np.array([[0.5, 0.0, 0.0, 0.0, 0.0, 0.0],
                   [0.0, 1.0, 0.0, 0.25, 0.0, 0.0],
                   [0.0, 0.0, 3.0, 0.0, 0.0, 0.0],
                   [0.1, 0.2, 0.3, 0.4, 0.0, 0.0],
                   [0.0, 0.0, 0.0, 1e-3, 0.0, 0.0],
                   [1.0, 0.0, 1.0, 0.0, 0.0, 0.0],
                   [0.0, 0.7, 0.0, 0.0, 0.0, 0.0],
                   [2.0, 0.0, 0.0, 0.05, 0.0, 0.0],
                   [0.0, 0.0, 0.0, 0.0, 0.0, 1.0 / 3.0]])


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
    return np.array([pm.population(d).toarray() for d in days])


def _assert_fields(P, ref):
    assert ref.shape[0] == P.nout
    for e in range(P.nout):
        got = P.field(e)
        assert got.dtype == np.float64 and got.shape == ref[e].shape
        assert np.array_equal(got, ref[e]), (e, np.abs(got - ref[e]).max())


@pytest.mark.parametrize('prob_model', [False, True])
@pytest.mark.parametrize('mode', ['exact', None])
def test_device_fields_match_the_numpy_reference_bit_for_bit(prob_model, mode):
    from parasitoids_amd.predictive import Projection, emergence_weights, exposure_weights
    pm = _pop_model(prob_model=prob_model, **({} if mode is None else {'mode': mode}))
    We = exposure_weights(DAYS, UPTO)
    Wd = emergence_weights(6, DAYS)                       # 25 outputs; those before day 13 carry no weight
    Wt = np.linspace(0.05, 1.0, 25 * 6).reshape(25, 6)    # 25 dense outputs: four output tiles, the last partial
    with Projection(pm, We, DAYS) as X, Projection(pm, Wd, DAYS) as D, Projection(pm, Wt, DAYS) as T:
        assert X.nout == 3 and D.nout == T.nout == 25 and X.N == 257
        assert D.live == list(range(13, 25)) and T.live == list(range(25))
        for mem in MEMBERS[:2]:                           # the second apply overwrites the first
            _evaluate(pm, mem)
            for P in (X, D, T):
                P.apply()
            f = _fields(pm, DAYS)
            assert f.max() > 0
            _assert_fields(X, project(f, We))
            _assert_fields(D, project(f, Wd))
            _assert_fields(T, project(f, Wt))
            assert np.array_equal(X.field(0), f[0]) and D.field(24).max() > 0 and not D.field(0).any()
        assert X.applies == 2
        rows, cols = np.array([128, 0, 256, 130, 128]), np.array([128, 0, 256, 117, 128])
        g = D.gather(rows, cols)
        assert g.shape == (25, 5)
        assert np.array_equal(g, np.array([D.field(e)[rows, cols] for e in range(25)]))
    pm.close()


def test_odd_cell_count_and_irregular_zero_pattern():
    """R = 64: N = 129, N * N odd, the last cell has a thread of its own; a dense hand-made matrix whose tiles
    skip some records and not others"""
    from parasitoids_amd.predictive import Projection
    pm = _pop_model(R=64)
    with Projection(pm, HAND_W, DAYS) as P:
        assert P.N == 129 and P.live == list(range(9))
        _evaluate(pm, MEMBERS[1])
        P.apply()
        f = _fields(pm, DAYS)
        ref = project(f, HAND_W)
        _assert_fields(P, ref)
        assert ref[8].max() > 0 and ref[4].max() > 0
        g = P.gather([128, 128, 64], [128, 127, 64])      # the tail cell and its neighbour
        assert np.array_equal(g, ref[:, [128, 128, 64], [128, 127, 64]])
    pm.close()


def locinfo_from(g):
    import pandas as pd
    td = lambda d: pd.Timedelta(days=int(d))
    li = types.SimpleNamespace()
    li.collection_datesPR = [td(d) for d in g['collection_days']]
    li.emerg_grids = [[tuple(rc) for rc in g['emerg_grid%d' % i]] for i in range(2)]
    li.release_DataFrames = [pd.DataFrame({'datePR': [td(d) for d in g['rel_dates%d' % i]]}) for i in range(2)]
    li.sent_DataFrames = [pd.DataFrame({'datePR': [td(d) for d in g['sen_dates%d' % i]]}) for i in range(2)]
    li.sent_ids = ['A', 'B', 'C']
    li.field_cells = {k: g['field_' + k] for k in li.sent_ids}
    li.grid_cells = g['grid_cells']
    li.grid_obs_datesPR = [td(d) for d in g['grid_obs_days']]
    li.card_obs_datesPR = [td(d) for d in g['card_obs_days']]
    li.card_obs = [np.zeros((4, int(n))) for n in g['card_obslen']]
    li.step_size = [int(v) for v in g['step_size']]
    return li


def _unique(days):
    out = []
    for d in days:
        if int(d) not in out:
            out.append(int(d))
    return out


def test_emergence_maps_reproduce_the_reference_numbers(golden, golden_dir):
    """G9: the reference's popdensity_to_emergence at collection days 3 and 6"""
    from parasitoids_amd import ParasitoidModel as PM, Bayes_funcs as BF
    from parasitoids_amd.pop_model import PopModel
    from parasitoids_amd.predictive import Projection, emergence_weights
    g = golden('g9_bayes_funcs')
    li = locinfo_from(g)
    wd, days = PM.get_wind_data(os.path.join(golden_dir, 'data', 'kalbar'), 30, '00:00')
    pm = PopModel(wd, days, domain_info=(10000.0, 128), r_number=130000, mode='exact')
    pm.evaluate(HP, DP, DLP, MU_R, NPER, ndays=6)
    rel, sen = BF.popdensity_to_emergence(pm, li)
    tol = dict(rtol=1e-10, atol=1e-9)
    for i in range(2):
        cday = int(g['collection_days'][i])
        assert cday == (3, 6)[i]
        with Projection(pm, emergence_weights(cday, range(6), _unique(g['rel_dates%d' % i])), range(6)) as P:
            P.apply()
            cells = np.asarray(g['emerg_grid%d' % i]).reshape(-1, 2)
            got = P.gather(cells[:, 0], cells[:, 1]).T
            assert got.shape == g['rel%d' % i].shape
            np.testing.assert_allclose(got, g['rel%d' % i], **tol)
            np.testing.assert_allclose(got, rel[i], **tol)
        with Projection(pm, emergence_weights(cday, range(6), _unique(g['sen_dates%d' % i])), range(6)) as P:
            P.apply()
            maps = [P.field(e) for e in range(P.nout)]
            got = np.array([[m[li.field_cells[k][:, 0], li.field_cells[k][:, 1]].sum() for m in maps]
                            for k in li.sent_ids])
            assert got.shape == g['sen%d' % i].shape
            np.testing.assert_allclose(got, g['sen%d' % i], **tol)
            np.testing.assert_allclose(got, sen[i], **tol)
    assert g['rel1'].max() > 0 and g['sen0'].max() > 1.0
    pm.close()


def _weighted_moments(Y, weights):
    """Y: [member, ...] -> (mean, population variance) with integer weights"""
    w = np.asarray(weights, dtype=np.float64).reshape((-1,) + (1,) * (Y.ndim - 1))
    mean = (w * Y).sum(0) / w.sum()
    return mean, (w * (Y - mean) ** 2).sum(0) / w.sum()


def test_posterior_of_a_sum_is_not_the_sum_of_posteriors():
    from parasitoids_amd.predictive import Projection, SpreadSummary, exposure_weights
    pm = _pop_model()
    W = exposure_weights(DAYS, [5])
    Y = []
    with Projection(pm, W, DAYS) as P, SpreadSummary.for_projection(P, THR) as S, SpreadSummary(pm, DAYS) as Sd:
        assert S.days == [0] and S.N == 257
        for mem, w in zip(MEMBERS, WEIGHTS):
            _evaluate(pm, mem)
            P.apply()
            S.add(w)
            Sd.add(w)
            Y.append(project(_fields(pm, DAYS), W)[0])
        Y = np.array(Y)
        Wt = float(sum(WEIGHTS))
        assert S.total_weight == Wt and S.members == len(MEMBERS)
        mean, var = _weighted_moments(Y, WEIGHTS)
        np.testing.assert_allclose(S.mean(0), mean, rtol=1e-12, atol=1e-12 * mean.max())
        got = S.variance(0)
        np.testing.assert_allclose(got, var, rtol=1e-9, atol=1e-12 * var.max())
        # the day-to-day covariances matter: the sum of the per-day variances is another number
        c = np.unravel_index(np.argmax(var), var.shape)
        day_sum = sum(Sd.variance(d)[c] for d in DAYS)
        assert abs(got[c] - day_sum) > 0.01 * got[c], (got[c], day_sum)
        for k, t in enumerate(THR):
            cnt = sum(w * (y >= t).astype(np.int64) for w, y in zip(WEIGHTS, Y))
            assert 0 < cnt.max() <= sum(WEIGHTS)
            assert np.array_equal(S.exceedance(0, k), cnt.astype(np.float64) / Wt), k
    pm.close()


def test_histogram_on_a_projection():
    from parasitoids_amd.predictive import Projection, SpreadHistogram, emergence_weights, exposure_weights
    pm = _pop_model()
    W = np.concatenate([exposure_weights(DAYS, UPTO), emergence_weights(6, DAYS)[[12, 13, 20]]])
    Y = []
    with Projection(pm, W, DAYS) as P, SpreadHistogram.for_projection(P) as H:
        assert P.live == [0, 1, 2, 4, 5] and H.days == list(range(6)) and H.edges.size == 225
        for mem, w in zip(MEMBERS, WEIGHTS):
            _evaluate(pm, mem)
            P.apply()
            H.add(w)
            Y.append(project(_fields(pm, DAYS), W))
        Y = np.array(Y)                                    # [member, output, N, N]
        assert H.total_weight == sum(WEIGHTS) and H.members == len(MEMBERS)
        for e in range(6):
            ref = weighted_counts(Y[:, e], WEIGHTS, H.edges)
            got = H.counts(e)
            assert got.dtype == np.uint32 and np.array_equal(got.astype(np.int64), ref), e
            for p in (0.05, 0.5, 0.95):
                q = exact_quantile(Y[:, e], WEIGHTS, p)
                lo, hi = H.quantile_bounds(e, p)
                assert np.all(lo <= q) and np.all(q < hi), (e, p)
        assert not Y[:, 3].any() and Y[:, 4].max() > 0     # output 3 carries no weight: all in bin 0
        assert np.array_equal(H.exceedance(2, H.edges[100]),
                              sum(w * (y >= H.edges[100]) for w, y in zip(WEIGHTS, Y[:, 2])) / float(sum(WEIGHTS)))
    pm.close()


def test_add_order_and_merge_order():
    from parasitoids_amd.predictive import Projection, SpreadHistogram, SpreadSummary, exposure_weights
    pm = _pop_model()
    W = exposure_weights(DAYS, UPTO)
    with Projection(pm, W, DAYS) as P:
        S = [SpreadSummary.for_projection(P, THR) for _ in range(4)]
        H = [SpreadHistogram.for_projection(P) for _ in range(4)]
        order = list(range(len(MEMBERS)))
        for i in order:
            _evaluate(pm, MEMBERS[i])
            P.apply()
            for acc in (S, H):
                acc[0].add(WEIGHTS[i])
                acc[2 if i < 2 else 3].add(WEIGHTS[i])
        for i in reversed(order):
            _evaluate(pm, MEMBERS[i])
            P.apply()
            S[1].add(WEIGHTS[i])
            H[1].add(WEIGHTS[i])
        S[3].merge(S[2])                                   # second half + first half
        H[2].merge(H[3])                                   # first half + second half
        for e in range(3):
            c = H[0].counts(e)
            assert np.array_equal(H[1].counts(e), c) and np.array_equal(H[2].counts(e), c)
            m = S[0].mean(e)
            for other in (S[1], S[3]):
                for k in range(len(THR)):
                    assert np.array_equal(other.exceedance(e, k), S[0].exceedance(e, k))
                np.testing.assert_allclose(other.mean(e), m, rtol=1e-12, atol=1e-12 * m.max())
        assert S[3].total_weight == S[0].total_weight and S[3].members == S[0].members
        for a in S + H:
            a.close()
    pm.close()


def test_members_on_different_cached_solvers_in_exact_mode():
    """the kernel extent moves with the diffusion parameters; in exact mode each extent has its own solver and
    stream, and successive applies and adds are ordered by the handles' events"""
    from parasitoids_amd.predictive import Projection, SpreadSummary, emergence_weights, exposure_weights
    W = np.concatenate([exposure_weights(DAYS, UPTO), emergence_weights(6, DAYS)[20:22]])
    mems = [((120.0, 100.0, 0.2), 1.0), ((260.0, 230.0, 0.25), 1.2), ((120.0, 100.0, 0.2), 1.05),
            ((200.0, 170.0, 0.1), 1.1)]
    w = [2, 1, 1, 3]
    pm = _pop_model(mode='exact')
    solvers = set()
    got = []
    with Projection(pm, W, DAYS) as P, SpreadSummary.for_projection(P) as S:
        for mem, wi in zip(mems, w):
            _evaluate(pm, mem)
            solvers.add(id(pm.solver))
            P.apply()
            S.add(wi)
        mean = [S.mean(e) for e in range(5)]
        for mem in mems:                                   # one apply per solver switch, read back each time
            _evaluate(pm, mem)
            P.apply()
            got.append(np.array([P.field(e) for e in range(5)]))
    assert len(solvers) >= 2
    pm.close()
    fresh = []
    for mem in mems:
        one = _pop_model(mode='exact')
        _evaluate(one, mem)
        with Projection(one, W, DAYS) as Q:
            Q.apply()
            f = np.array([Q.field(e) for e in range(5)])
        assert np.array_equal(f, project(_fields(one, DAYS), W))
        fresh.append(f)
        one.close()
    for a, b in zip(got, fresh):
        assert np.array_equal(a, b)
    ref, _ = _weighted_moments(np.array(fresh), w)
    for e in range(5):
        np.testing.assert_allclose(mean[e], ref[e], rtol=1e-12, atol=1e-12 * ref[e].max())


def _all_maps(S, H, days, nthr):
    out = []
    for d in days:
        out += [S.mean(d), S.variance(d)] + [S.exceedance(d, k) for k in range(nthr)]
        out += [H.counts(d), H.quantile(d, 0.5)]
    return out


def test_day_based_accumulators_are_untouched_by_projection_adds():
    """each pass starts from a fresh PopModel: an auto-mode model routes days by what it has seen before, which
    may move a field by rounding"""
    from parasitoids_amd.predictive import Projection, SpreadHistogram, SpreadSummary, exposure_weights
    pm = _pop_model()
    days = [0, 3, 5]
    W = exposure_weights(DAYS, UPTO)
    with SpreadSummary(pm, days, THR) as S0, SpreadHistogram(pm, days) as H0:
        for mem, w in zip(MEMBERS, WEIGHTS):
            _evaluate(pm, mem)
            S0.add(w)
            H0.add(w)
        alone = _all_maps(S0, H0, days, len(THR))
    pm.close()
    pm = _pop_model()
    with SpreadSummary(pm, days, THR) as S, SpreadHistogram(pm, days) as H, Projection(pm, W, DAYS) as P, \
            SpreadSummary.for_projection(P, THR) as SP, SpreadHistogram.for_projection(P) as HP_:
        for mem, w in zip(MEMBERS, WEIGHTS):
            _evaluate(pm, mem)
            S.add(w)
            P.apply()
            SP.add(w)
            H.add(w)
            HP_.add(w)
        along = _all_maps(S, H, days, len(THR))
        assert SP.total_weight == S.total_weight == sum(WEIGHTS)
    assert len(alone) == len(along)
    for a, b in zip(alone, along):
        assert np.array_equal(a, b)
    pm.close()


def test_refusals_and_the_handles_stay_usable():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import NEGVAL, Projection, SpreadHistogram, SpreadSummary, exposure_weights
    lib = L.load()
    dev = L.default_device()
    h = L._VP()

    def create(W, N=257):
        W = L.f64(W)
        return lib.ps_project_create(dev, N, W.shape[1], W.shape[0], L.p_f64(W), C.byref(h))
    assert create(np.ones((2, 33))) == L.PS_ERR_BAD_ARG and not h
    assert create(np.ones((33, 2))) == L.PS_ERR_BAD_ARG and not h
    for bad in (-1.0, np.nan, np.inf):
        assert create([[1.0, bad], [1.0, 1.0]]) == L.PS_ERR_BAD_ARG and not h
    assert create([[1.0, 0.0], [0.0, 0.0]]) == L.PS_ERR_BAD_ARG and not h
    assert b'no non-zero weight' in lib.ps_last_error()
    assert create(np.ones((32, 32)), N=60001) == L.PS_ERR_OOM and not h       # 0.9 TB of outputs
    assert b'GB free' in lib.ps_last_error()
    W = exposure_weights(DAYS, UPTO)
    pm, small = _pop_model(), _pop_model(R=64)
    with Projection(pm, W, DAYS) as P, Projection(small, W, DAYS) as P64, \
            SpreadSummary.for_projection(P, THR) as S, SpreadHistogram.for_projection(P) as H, \
            SpreadSummary(pm, [0, 1]) as S2, SpreadHistogram(pm, [0, 1]) as H2:
        with pytest.raises(ValueError):
            P.apply()                                      # nothing evaluated yet
        _evaluate(pm, MEMBERS[0])
        _evaluate(small, MEMBERS[0])
        for acc in (S, H):
            with pytest.raises(L.HipError) as err:
                acc.add(1)                                 # nothing projected yet
            assert err.value.code == L.PS_ERR_STATE
        with pytest.raises(L.HipError) as err:
            P.field(0)
        assert err.value.code == L.PS_ERR_STATE
        P.apply()
        P64.apply()
        # slot count: 3 outputs into 2 slots; domain: 129 x 129 outputs into 257 x 257 slots
        assert lib.ps_summary_add_project(S2._h, P._h, 1) == L.PS_ERR_BAD_ARG
        assert lib.ps_hist_add_project(H2._h, P._h, 1) == L.PS_ERR_BAD_ARG
        assert lib.ps_summary_add_project(S._h, P64._h, 1) == L.PS_ERR_BAD_ARG
        assert lib.ps_hist_add_project(H._h, P64._h, 1) == L.PS_ERR_BAD_ARG
        assert lib.ps_summary_add_project(S._h, P._h, 0) == L.PS_ERR_BAD_ARG
        kind, idx, delta = L.i32([L.REC_STATE] * 6), L.i32([0] * 6), L.i32([0] * 6)
        one = L.f64([1.0] * 6)
        rc = lib.ps_project_apply(P._h, small.solver._h, 6, L.p_i32(kind), L.p_i32(idx), L.p_f64(one), L.p_f64(one),
                                  L.p_i32(delta), NEGVAL)
        assert rc == L.PS_ERR_BAD_ARG                      # a solver of another domain
        rc = lib.ps_project_apply(P._h, pm.solver._h, 5, L.p_i32(kind), L.p_i32(idx), L.p_f64(one), L.p_f64(one),
                                  L.p_i32(delta), NEGVAL)
        assert rc == L.PS_ERR_BAD_ARG                      # five records for six inputs
        with pytest.raises(L.HipError):
            P.gather([257], [0])                           # a cell outside the domain
        with pytest.raises(ValueError):
            P.field(3)
        for acc in (S, H, S2, H2):
            assert acc.members == 0 and acc.total_weight == 0
        assert P.applies == 1
        # nothing was enqueued and every handle still works
        ref = project(_fields(pm, DAYS), W)
        _assert_fields(P, ref)
        S.add(2)
        H.add(2)
        S2.add(1)
        assert S.members == 1 and S.total_weight == 2 and H.total_weight == 2
        for e in range(3):
            assert np.array_equal(S.mean(e), ref[e]) and not S.variance(e).any()
            assert np.array_equal(H.counts(e).astype(np.int64), weighted_counts([ref[e]], [2], H.edges))
        assert np.array_equal(S2.mean(1), _fields(pm, [1])[0])
    pm.close()
    small.close()


def _csr(f, key, N):
    from scipy import sparse
    return sparse.csr_matrix((f[key + '_data'], f[key + '_ind'], f[key + '_indptr']), shape=(N, N)).toarray()


def test_posterior_predictive_with_emergence_and_exposure(tmp_path):
    from parasitoids_amd import mcmc
    from parasitoids_amd.predictive import emergence_weights, exposure_weights, posterior_predictive
    pm = _pop_model()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        li = mcmc.synthetic_locinfo(pm, 128, seed=9, ndays=6)
        smp = mcmc.Sampler(pm, li, (10000.0 / 128) ** 2, seed=21, ndays=6)
        smp.run(40)
        smp.save(tmp_path / 'chain.npz')
        f = np.load(tmp_path / 'chain.npz')
        trace, names = f['trace'], [str(n) for n in f['names']]
        assert len(trace) == 40
        chains = [(trace[:25], names), (trace[25:], names)]
        kw = dict(thresholds=(1.0,), quantiles=[0.5])
        # a fresh model per call: an auto-mode model routes days by what it has seen before, which may move
        # a field by rounding, and the main files are compared bit for bit
        pa, pb = _pop_model(), _pop_model()
        res = posterior_predictive(pa, chains, emergence=dict(collection_day=6), exposure=[2, 5], **kw)
        plain = posterior_predictive(pb, chains, **kw)
    assert plain.emergence is None and plain.exposure is None
    em, ex = res.emergence, res.exposure
    assert em.labels == list(range(6, 31)) and ex.labels == [2, 5] and em.in_days == ex.in_days == DAYS
    assert np.array_equal(em.weights, emergence_weights(6, DAYS)) and np.array_equal(ex.weights, exposure_weights(DAYS, [2, 5]))
    for pr in (em, ex):
        assert pr.summary.total_weight == res.summary.total_weight > 0
        assert pr.summary.members == res.summary.members == len(res.runs)
        assert pr.histogram.total_weight == res.histogram.total_weight
    # by hand: every run once more, projected by the numpy reference
    cols = [names.index(m[0]) for m in mcmc.MODEL_BLOCK]
    sums = {'em': 0.0, 'ex': 0.0}
    Wt = 0
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        for ci, first, weight in res.runs:
            pm.evaluate(*mcmc.model_args(chains[ci][0][first, cols]), want_stats=False)
            fld = _fields(pm, DAYS)
            sums['em'] = sums['em'] + weight * project(fld, em.weights)
            sums['ex'] = sums['ex'] + weight * project(fld, ex.weights)
            Wt += weight
    assert Wt == res.summary.total_weight
    for key, pr in (('em', em), ('ex', ex)):
        ref = sums[key] / Wt
        assert ref.max() > 0
        for e in range(len(pr.labels)):
            np.testing.assert_allclose(pr.summary.mean(e), ref[e], rtol=1e-12, atol=1e-12 * ref.max())
    assert not em.summary.mean(0).any() and em.summary.mean(24).max() > 0
    npz, js = res.save(str(tmp_path / 'a' / 'pp'))
    npz_p, js_p = plain.save(str(tmp_path / 'p' / 'pp'))
    assert not os.path.exists(str(tmp_path / 'p' / 'pp_emergence.npz'))
    with np.load(npz) as fa, np.load(npz_p) as fp:
        assert set(fa.files) == set(fp.files)
        for k in fp.files:
            assert np.array_equal(fa[k], fp[k]), k
    N = 257
    for name, pr in (('emergence', em), ('exposure', ex)):
        with np.load(str(tmp_path / 'a' / ('pp_%s.npz' % name))) as fz:
            assert [int(x) for x in fz['days']] == pr.labels
            want = {'days'}
            for e, lab in enumerate(pr.labels):
                for suffix, m in (('', pr.summary.mean(e)), ('_sd', pr.summary.sd(e)),
                                  ('_pexc0', pr.summary.exceedance(e, 0)), ('_q50', pr.histogram.quantile(e, 0.5))):
                    assert np.array_equal(_csr(fz, '%d%s' % (lab, suffix), N), np.where(m >= 1e-8, m, 0.0)), (lab, suffix)
                    want |= {'%d%s_%s' % (lab, suffix, t) for t in ('data', 'ind', 'indptr')}
            assert set(fz.files) == want
    meta = json.load(open(js))['predictive']
    assert np.array_equal(meta['emergence']['weights'], em.weights) and meta['emergence']['in_days'] == DAYS
    assert meta['exposure']['labels'] == [2, 5] and meta['exposure']['weights'] == ex.weights.tolist()
    assert 'emergence' not in json.load(open(js_p))['predictive']
    for r in (res, plain):
        r.summary.close()
        r.histogram.close()
    em.close()
    ex.close()
    for p in (pm, pa, pb):
        p.close()
