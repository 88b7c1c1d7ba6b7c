"""GPU tests of the posterior predictive histograms (ps_hist_*, predictive.SpreadHistogram): the device
counts against a numpy weighted histogram of `PopModel.population(d)`, quantile brackets and point maps,
exceedance at edges, weights, merge and add order, solver switches, the memory check, and
posterior_predictive with quantile levels.  Kalbar wind, R = 128, 6 days, the members and weights of
test_predictive_gpu.py."""
import os
import warnings

import numpy as np
import pytest

from helpers import HP, DP, DLP, MU_R, NPER
from hist_ref import exact_quantile, exceedance_from_counts, quantile_from_counts, weighted_counts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.abspath(__file__))
MEMBERS = [(DP, MU_R), ((160.0, 150.0, 0.2), 1.1), ((185.0, 140.0, 0.3), 1.25), ((171.82, 160.0, 0.1), 1.0),
           ((150.0, 135.0, 0.28), 1.15)]
WEIGHTS = [1, 3, 1, 2, 1]
LEVELS = (0.05, 0.5, 0.95, 1.0)


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


def _edges_with_field_values(fields, bins):
    """the edges of bins plus values that occur in a member's field: those must land in the upper bin"""
    from parasitoids_amd.predictive import bin_edges
    f = np.asarray(fields[1][3])
    pos = np.sort(f[f > 0])
    picks = pos[np.linspace(0, pos.size - 1, 12).astype(int)]
    e = np.unique(np.concatenate([bin_edges(bins), picks]))
    return e, picks


@pytest.mark.parametrize('prob_model', [False, True])
def test_counts_quantiles_and_exceedance_match_numpy(prob_model):
    """exact mode: the second evaluation of a member gives the same field as the first, whose values
    made the extra edges"""
    from parasitoids_amd.predictive import SpreadHistogram, SpreadSummary
    pm = _pop_model(prob_model=prob_model, mode='exact')
    days = list(range(6))
    first = []
    for mem in MEMBERS:
        _evaluate(pm, mem)
        first.append(_fields(pm, days))
    edges, picks = _edges_with_field_values(first, (1e-8, 1e6, 8))
    k_thr = [int(np.searchsorted(edges, t)) for t in (picks[3], picks[8])]
    with SpreadHistogram(pm, days) as H, SpreadHistogram(pm, days, edges=edges) as E, \
            SpreadSummary(pm, days, [edges[k] for k in k_thr]) as S:
        fields = []
        for mem, w in zip(MEMBERS, WEIGHTS):
            _evaluate(pm, mem)
            H.add(w)
            E.add(w)
            S.add(w)
            fields.append(_fields(pm, days))
        assert H.total_weight == E.total_weight == sum(WEIGHTS) and H.members == len(MEMBERS)
        assert H.edges.size == 225 and np.array_equal(E.edges, edges)
        for i, d in enumerate(days):
            X = [f[i] for f in fields]
            for G in (H, E):
                ref = weighted_counts(X, WEIGHTS, G.edges)
                got = G.counts(d)
                assert got.dtype == np.uint32 and got.shape == ref.shape
                assert np.array_equal(got.astype(np.int64), ref), (d, G.edges.size)
                for p in LEVELS:
                    q = exact_quantile(X, WEIGHTS, p)
                    _b, val, lo, hi = quantile_from_counts(ref, G.edges, p)
                    glo, ghi = G.quantile_bounds(d, p)
                    assert np.array_equal(glo, lo) and np.array_equal(ghi, hi), (d, p)
                    assert np.all(glo <= q) and np.all(q < ghi), (d, p)
                    np.testing.assert_allclose(G.quantile(d, p), val, rtol=1e-12, atol=0)
            # exceedance at edges: numpy's weighted fraction, and the summary's bits at the same thresholds
            for k in [0, 30, 60, 90, E.edges.size - 1] + k_thr:
                ref = np.tensordot(np.asarray(WEIGHTS), (np.asarray(X) >= E.edges[k]).astype(np.int64), axes=1) \
                    / float(sum(WEIGHTS))
                got = E.exceedance(d, E.edges[k])
                assert np.array_equal(got, ref), (d, k)
                assert np.array_equal(got, exceedance_from_counts(E.counts(d), k))
            for j, k in enumerate(k_thr):
                assert np.array_equal(E.exceedance(d, E.edges[k]), S.exceedance(d, j)), (d, k)
        # edges that are field values: the cells holding exactly that value count in the upper bin
        on_edge = np.isin(fields[1][3], picks)
        assert on_edge.any()
        with pytest.raises(ValueError):
            H.exceedance(3, 3.0)                       # not an edge of the default table
    pm.close()


def test_weight_three_equals_three_unit_adds():
    from parasitoids_amd.predictive import SpreadHistogram
    pm = _pop_model()
    with SpreadHistogram(pm) as A, SpreadHistogram(pm) as B:
        for mem, n in zip(MEMBERS[:3], (1, 3, 2)):
            _evaluate(pm, mem)
            A.add(n)
            for _ in range(n):
                B.add(1)
        assert A.total_weight == B.total_weight == 6 and B.members == 6
        for d in A.days:
            assert np.array_equal(A.counts(d), B.counts(d))
            for p in (0.05, 0.5):
                assert np.array_equal(A.quantile(d, p), B.quantile(d, p))
    pm.close()


def test_merge_order_and_add_order_do_not_change_a_bit():
    from parasitoids_amd.predictive import SpreadHistogram
    pm = _pop_model()
    days = [0, 2, 5]
    hs = [SpreadHistogram(pm, days) for _ in range(6)]
    fwd, rev, a1, b1, a2, b2 = hs
    order = list(range(len(MEMBERS)))
    for i in order:
        _evaluate(pm, MEMBERS[i])
        fwd.add(WEIGHTS[i])
        (a1 if i < 2 else b1).add(WEIGHTS[i])
        (a2 if i < 2 else b2).add(WEIGHTS[i])
    for i in reversed(order):
        _evaluate(pm, MEMBERS[i])
        rev.add(WEIGHTS[i])
    a1.merge(b1)              # first half + second half
    b2.merge(a2)              # second half + first half
    for d in days:
        c = fwd.counts(d)
        for other in (rev, a1, b2):
            assert np.array_equal(other.counts(d), c)
            assert np.array_equal(other.quantile(d, 0.5), fwd.quantile(d, 0.5))
            assert np.array_equal(other.exceedance(d, fwd.edges[160]), fwd.exceedance(d, fwd.edges[160]))
    assert a1.members == b2.members == fwd.members and a1.total_weight == fwd.total_weight
    with SpreadHistogram(pm, days) as e:             # merging into an empty histogram
        e.merge(fwd)
        assert all(np.array_equal(e.counts(d), fwd.counts(d)) for d in days)
    with SpreadHistogram(pm, days, bins=(1e-8, 1e6, 8)) as other, pytest.raises(Exception):
        fwd.merge(other)                             # different edges
    for h in hs:
        h.close()
    pm.close()


def test_members_on_different_cached_solvers_in_exact_mode():
    """the kernel extent moves with the diffusion parameters; in exact mode each extent has its own
    solver and stream, and successive adds from them are ordered by the histogram's event"""
    from parasitoids_amd.predictive import SpreadHistogram
    pm = _pop_model(mode='exact')
    mems = [((120.0, 100.0, 0.2), 1.0), ((260.0, 230.0, 0.25), 1.2), ((120.0, 100.0, 0.2), 1.05),
            ((200.0, 170.0, 0.1), 1.1)]
    w = [2, 1, 1, 3]
    days = list(range(6))
    solvers = set()
    with SpreadHistogram(pm, days) as H:
        for mem, wi in zip(mems, w):
            _evaluate(pm, mem)
            solvers.add(id(pm.solver))
            H.add(wi)
        fields = []
        for mem in mems:       # read back only now: every add was enqueued behind the next evaluation
            _evaluate(pm, mem)
            fields.append(_fields(pm, days))
        assert len(solvers) >= 2
        for i, d in enumerate(days):
            X = [f[i] for f in fields]
            ref = weighted_counts(X, w, H.edges)
            assert np.array_equal(H.counts(d).astype(np.int64), ref), d
            _b, val, lo, hi = quantile_from_counts(ref, H.edges, 0.5)
            np.testing.assert_allclose(H.quantile(d, 0.5), val, rtol=1e-12, atol=0)
    pm.close()


def test_out_of_memory_is_reported_and_the_device_stays_usable():
    import ctypes as C
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import SpreadHistogram, bin_edges
    lib = L.load()
    e = bin_edges((1e-8, 1e6, 64))                  # 897 edges
    h = L._VP()
    rc = lib.ps_hist_create(L.default_device(), 8001, 60, e.size, L.p_f64(e), C.byref(h))   # ~14 TB
    assert rc == L.PS_ERR_OOM and not h
    assert b'GB free' in lib.ps_last_error()
    pm = _pop_model()
    _evaluate(pm, MEMBERS[0])
    with SpreadHistogram(pm, [1, 4]) as H:
        H.add(2)
        X = _fields(pm, [1, 4])
        for i, d in enumerate([1, 4]):
            assert np.array_equal(H.counts(d).astype(np.int64), weighted_counts([X[i]], [2], H.edges))
        assert lib.ps_hist_exceed(H._h, 2, 0, L.p_f64(np.empty(257 * 257))) == L.PS_ERR_BAD_ARG   # bad slot
    with SpreadHistogram(pm, [1]) as H, pytest.raises(L.HipError) as err:
        H.quantile(1, 0.5)                           # nothing accumulated
    assert err.value.code == L.PS_ERR_STATE
    pm.close()


def _split_chain(tmp_path):
    from parasitoids_amd import mcmc
    pm = _pop_model(ndays=18)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        li = mcmc.synthetic_locinfo(pm, 128, seed=9)
        smp = mcmc.Sampler(pm, li, (10000.0 / 128) ** 2, seed=21)
        smp.run(12)
    smp.save(tmp_path / 'chain.npz')
    pm.close()
    f = np.load(tmp_path / 'chain.npz')
    tr, names = f['trace'], [str(n) for n in f['names']]
    return (tr[:6], names), (tr[6:], names)


def _keys(npz):
    with np.load(npz) as f:
        return set(f.files)


def test_posterior_predictive_with_quantiles(tmp_path):
    from parasitoids_amd.predictive import posterior_predictive
    c1, c2 = _split_chain(tmp_path)
    days = [0, 4, 9, 17]
    levels = [0.05, 0.5, 0.95]
    one = _pop_model(ndays=18, mode='exact')
    pa, pb = _pop_model(ndays=18, mode='exact'), _pop_model(ndays=18, mode='exact')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        r1 = posterior_predictive(one, [c1, c2], days=days, thresholds=(1.0,), quantiles=levels)
        r2 = posterior_predictive([pa, pb], [c1, c2], days=days, thresholds=(1.0,), quantiles=levels)
        plain = posterior_predictive(one, [c1, c2], days=days, thresholds=(1.0,))
    assert r1.quantiles == r2.quantiles == levels and plain.histogram is None and plain.quantiles is None
    for r in (r1, r2):
        assert r.histogram.total_weight == r.summary.total_weight > 0
        assert r.histogram.members == r.summary.members == r.evaluations - r.failed
    for d in days:
        assert np.array_equal(r1.histogram.counts(d), r2.histogram.counts(d))
        for p in levels:
            q = r1.histogram.quantile(d, p)
            assert np.array_equal(q, r2.histogram.quantile(d, p))
            lo, hi = r1.histogram.quantile_bounds(d, p)
            assert np.all((lo <= q) & (q <= hi))
    npz_q, js_q = r1.save(str(tmp_path / 'q' / 'pp'))
    npz_p, js_p = plain.save(str(tmp_path / 'p' / 'pp'))
    labels = [str(one.days[d]) for d in days]
    old = {'days'} | {'%s%s_%s' % (lab, s, t) for lab in labels for s in ('', '_sd', '_pexc0')
                      for t in ('data', 'ind', 'indptr')}
    assert _keys(npz_p) == old
    qk = {'%s_%s_%s' % (lab, q, t) for lab in labels for q in ('q5', 'q50', 'q95') for t in ('data', 'ind', 'indptr')}
    assert _keys(npz_q) == old | qk
    from scipy import sparse
    N = 257
    with np.load(npz_q) as f:
        lab = labels[2]
        M = sparse.csr_matrix((f[lab + '_q50_data'], f[lab + '_q50_ind'], f[lab + '_q50_indptr']), shape=(N, N))
        m = r1.histogram.quantile(days[2], 0.5)
        assert np.array_equal(M.toarray(), np.where(m >= 1e-8, m, 0.0))
    import json
    meta = json.load(open(js_q))
    assert meta['predictive']['quantiles']['levels'] == levels
    assert 'quantiles' not in json.load(open(js_p))['predictive']
    for r in (r1, r2, plain):
        r.summary.close()
        if r.histogram is not None:
            r.histogram.close()
    for p in (one, pa, pb):
        p.close()
