"""GPU tests of the posterior arrival maps (ps_arrival_*, predictive.ArrivalMaps): device counts, arrival
probabilities, arrival quantiles and reached-cell rows against the numpy reference built from
`PopModel.population(d)`, the tie to SpreadSummary's exceedance, weights, merge and add order, solver
switches, day subsets, the refusals, and posterior_predictive with arrival thresholds.  Kalbar wind,
R = 128, 6 days, the members and weights of test_spread_histogram_gpu.py."""
import os
import warnings

import numpy as np
import pytest

from helpers import HP, DP, DLP, MU_R, NPER
from arrival_ref import probability, quantile_slots, reached_rows, weighted_counts, cumulative

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.abspath(__file__))
MEMBERS = [(DP, MU_R), ((160.0, 150.0, 0.2), 1.1), ((185.0, 140.0, 0.3), 1.25), ((171.82, 160.0, 0.1), 1.0),
           ((150.0, 135.0, 0.28), 1.15)]
WEIGHTS = [1, 3, 1, 2, 1]
THR = [1.0, 10.0]
THR4 = [1e-4, 1.0, 10.0, 100.0]
LEVELS = (0.05, 0.3, 0.5, 0.95, 1.0)


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


def _check_against_reference(A, fields, weights, thr):
    """every device output of A against the numpy reference of the members' [nslot, N, N] fields"""
    days = A.days
    ref = weighted_counts(fields, weights, thr)
    P = probability(ref)
    rows = reached_rows(fields, thr)
    for k in range(len(thr)):
        for s, d in enumerate(days):
            got = A.counts(k, d)
            assert got.dtype == np.uint32 and got.shape == ref.shape[2:]
            assert np.array_equal(got.astype(np.int64), ref[k, s]), (k, d)
            assert np.array_equal(A.prob_by(k, d), P[k, s]), (k, d)
        assert np.array_equal(A.counts(k, None).astype(np.int64), ref[k, -1]), k
        for p in LEVELS:
            q = quantile_slots(ref, p)[k]
            want = np.where(q < 0, -1, np.asarray(days)[q.clip(0)])
            got = A.quantile(k, p)
            assert got.dtype == np.int32 and np.array_equal(got, want), (k, p)
        cells, w = A.reached(k)
        assert np.array_equal(cells, rows[:, k, :]), k
        assert w.tolist() == list(weights)
        # the exact tie between the two device outputs: sum_m w_m n_k^m(s) == sum_c C_k[s](c)
        lhs = (cells * w[:, None]).sum(0)
        rhs = np.array([sum(int(A.counts(k, dd).astype(np.int64).sum()) for dd in days[:s + 1])
                        for s in range(len(days))])
        assert np.array_equal(lhs, rhs) and np.array_equal(lhs, cumulative(ref)[k].reshape(len(days), -1).sum(1))
    return ref


@pytest.mark.parametrize('prob_model', [False, True])
@pytest.mark.parametrize('mode', ['exact', None])
def test_device_maps_match_the_numpy_reference(prob_model, mode):
    from parasitoids_amd.predictive import ArrivalMaps, SpreadSummary
    pm = _pop_model(prob_model=prob_model, **({} if mode is None else {'mode': mode}))
    days = list(range(6))
    scale = 1.0 / 130000 if prob_model else 1.0     # prob_model holds probabilities: the same densities
    thr, thr4 = [t * scale for t in THR], [t * scale for t in THR4]
    fields = []
    with ArrivalMaps(pm, thr) as A, ArrivalMaps(pm, thr4, days) as A4, SpreadSummary(pm, days, thr) as S:
        assert A.days == days and A.N == 257 and A.cell_area == (10000.0 / 128) ** 2
        for mem, w in zip(MEMBERS, WEIGHTS):
            _evaluate(pm, mem)
            A.add(w)
            A4.add(w)
            S.add(w)
            fields.append(_fields(pm, days))
        assert A.total_weight == sum(WEIGHTS) and A.members == len(MEMBERS)
        ref = _check_against_reference(A, fields, WEIGHTS, thr)
        assert ref[1, :-1].sum() > 0 and ref[1, :-1].sum() < ref[0, :-1].sum()   # the plume reaches both
        _check_against_reference(A4, fields, WEIGHTS, thr4)
        for k in range(len(thr)):
            assert np.array_equal(A.prob_by(k, days[0]), S.exceedance(days[0], k)), k
            prev = None
            for d in days:
                p = A.prob_by(k, d)
                assert np.all(p >= S.exceedance(d, k)), (k, d)
                if prev is not None:
                    assert np.all(p >= prev), (k, d)
                prev = p
        for d in days:
            assert np.all(A.prob_by(1, d) <= A.prob_by(0, d))
    pm.close()


def test_weight_three_equals_three_unit_adds():
    from parasitoids_amd.predictive import ArrivalMaps
    pm = _pop_model()
    with ArrivalMaps(pm, THR) as A, ArrivalMaps(pm, THR) as B:
        for mem, n in zip(MEMBERS[:3], (1, 3, 2)):
            _evaluate(pm, mem)
            A.add(n)
            for _ in range(n):
                B.add(1)
        assert A.total_weight == B.total_weight == 6 and A.members == 3 and B.members == 6
        for k in range(2):
            for d in A.days + [None]:
                assert np.array_equal(A.counts(k, d), B.counts(k, d))
            for p in (0.05, 0.5, 1.0):
                assert np.array_equal(A.quantile(k, p), B.quantile(k, p))
            ca, wa = A.reached(k)
            cb, wb = B.reached(k)
            assert np.array_equal(np.repeat(ca, wa, axis=0), cb) and wb.tolist() == [1] * 6
            assert [r['quantiles'] for r in A.reached_area(k)] == [r['quantiles'] for r in B.reached_area(k)]
    pm.close()


def test_merge_order_and_add_order_do_not_change_a_bit():
    from parasitoids_amd.predictive import ArrivalMaps
    pm = _pop_model()
    days = [0, 2, 5]
    hs = [ArrivalMaps(pm, THR, days) for _ in range(6)]
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
    for k in range(2):
        for d in days + [None]:
            c = fwd.counts(k, d)
            for other in (rev, a1, b2):
                assert np.array_equal(other.counts(k, d), c)
        for d in days:
            for other in (rev, a1, b2):
                assert np.array_equal(other.prob_by(k, d), fwd.prob_by(k, d))
        for other in (rev, a1, b2):
            assert np.array_equal(other.quantile(k, 0.5), fwd.quantile(k, 0.5))
        cf, wf = fwd.reached(k)
        cr, wr = rev.reached(k)
        assert np.array_equal(cr, cf[::-1]) and wr.tolist() == wf.tolist()[::-1]
        c1, w1 = a1.reached(k)
        assert np.array_equal(c1, cf) and w1.tolist() == wf.tolist()      # merge appends in order
        c2, w2 = b2.reached(k)
        assert np.array_equal(c2, np.concatenate([cf[2:], cf[:2]])) and w2.tolist() == wf.tolist()[2:] + wf.tolist()[:2]
    assert a1.members == b2.members == fwd.members and a1.total_weight == fwd.total_weight
    with ArrivalMaps(pm, THR, days) as e:             # merging into an empty handle
        e.merge(fwd)
        assert all(np.array_equal(e.counts(0, d), fwd.counts(0, d)) for d in days)
        assert np.array_equal(e.reached(0)[0], fwd.reached(0)[0])
    with ArrivalMaps(pm, [1.0, 20.0], days) as other, pytest.raises(Exception):
        fwd.merge(other)                             # different thresholds
    for h in hs:
        h.close()
    pm.close()


def test_many_members_grow_the_rows_without_changing_them():
    """more members than the first row block: the rows double and keep what they held"""
    from parasitoids_amd.predictive import ArrivalMaps
    pm = _pop_model(ndays=3)
    fields = []
    with ArrivalMaps(pm, THR) as A:
        for r in range(70):
            if r < len(MEMBERS):
                _evaluate(pm, MEMBERS[r])
                fields.append(_fields(pm, A.days))
            A.add(1 + r % 3)
        rows = reached_rows(fields, THR)
        cells, w = A.reached(0)
        assert cells.shape == (70, 3) and np.array_equal(cells[:5], rows[:, 0]) and np.all(cells[5:] == rows[-1, 0])
        assert w.tolist() == [1 + r % 3 for r in range(70)]
    pm.close()


def test_members_on_different_cached_solvers_in_exact_mode():
    """the kernel extent moves with the diffusion parameters; in exact mode each extent has its own
    solver and stream, and successive adds from them are ordered by the handle's event"""
    from parasitoids_amd.predictive import ArrivalMaps
    pm = _pop_model(mode='exact')
    mems = [((120.0, 100.0, 0.2), 1.0), ((260.0, 230.0, 0.25), 1.2), ((120.0, 100.0, 0.2), 1.05),
            ((200.0, 170.0, 0.1), 1.1)]
    w = [2, 1, 1, 3]
    solvers = set()
    with ArrivalMaps(pm, THR) as A:
        for mem, wi in zip(mems, w):
            _evaluate(pm, mem)
            solvers.add(id(pm.solver))
            A.add(wi)
        fields = []
        for mem in mems:       # read back only now: every add was enqueued behind the next evaluation
            _evaluate(pm, mem)
            fields.append(_fields(pm, A.days))
        assert len(solvers) >= 2
        _check_against_reference(A, fields, w, THR)
    pm.close()


def test_a_day_subset_observes_arrival_on_the_listed_days_only():
    from parasitoids_amd.predictive import ArrivalMaps
    pm = _pop_model()
    sub = [0, 2, 5]
    fields = []
    with ArrivalMaps(pm, THR, sub) as A, ArrivalMaps(pm, THR) as F:
        for mem, w in zip(MEMBERS, WEIGHTS):
            _evaluate(pm, mem)
            A.add(w)
            F.add(w)
            fields.append(_fields(pm, sub))
        _check_against_reference(A, fields, WEIGHTS, THR)
        # the subset sees no arrival on the days it skips: reached by d on a listed day implies reached by d
        for k in range(2):
            assert np.array_equal(A.prob_by(k, 0), F.prob_by(k, 0))
            for d in sub:
                assert np.all(A.prob_by(k, d) <= F.prob_by(k, d)), (k, d)
    pm.close()


def test_refusals_and_the_device_stays_usable():
    import ctypes as C
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import ArrivalMaps
    lib = L.load()
    dev = L.default_device()
    h = L._VP()
    thr5 = L.f64([1.0, 2.0, 3.0, 4.0, 5.0])
    assert lib.ps_arrival_create(dev, 257, 33, 2, L.p_f64(thr5), C.byref(h)) == L.PS_ERR_BAD_ARG and not h
    assert lib.ps_arrival_create(dev, 257, 6, 5, L.p_f64(thr5), C.byref(h)) == L.PS_ERR_BAD_ARG and not h
    assert lib.ps_arrival_create(dev, 257, 6, 2, L.p_f64(L.f64([2.0, 1.0])), C.byref(h)) == L.PS_ERR_BAD_ARG
    rc = lib.ps_arrival_create(dev, 40001, 32, 4, L.p_f64(thr5), C.byref(h))      # ~0.8 TB
    assert rc == L.PS_ERR_OOM and not h
    assert b'GB free' in lib.ps_last_error()
    pm = _pop_model()
    _evaluate(pm, MEMBERS[0])
    with ArrivalMaps(pm, THR, [1, 4]) as A:
        with pytest.raises(L.HipError) as err:
            A.quantile(0, 0.5)                       # nothing accumulated
        assert err.value.code == L.PS_ERR_STATE
        A.add(2)
        X = _fields(pm, [1, 4])
        _check_against_reference(A, [X], [2], THR)
        A.reset()
        assert A.members == 0 and A.total_weight == 0
        with pytest.raises(L.HipError) as err:
            A.prob_by(0, 1)
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


def test_posterior_predictive_with_arrival_maps(tmp_path):
    from scipy import sparse
    from parasitoids_amd.predictive import posterior_predictive
    c1, c2 = _split_chain(tmp_path)
    days = [0, 4, 9, 17]
    one = _pop_model(ndays=18, mode='exact')
    pa, pb = _pop_model(ndays=18, mode='exact'), _pop_model(ndays=18, mode='exact')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        r1 = posterior_predictive(one, [c1, c2], days=days, thresholds=(1.0,), arrival=[1, 10])
        r2 = posterior_predictive([pa, pb], [c1, c2], days=days, thresholds=(1.0,), arrival=[1, 10])
        plain = posterior_predictive(one, [c1, c2], days=days, thresholds=(1.0,))
    assert plain.arrival is None and plain.arrival_levels is None
    assert r1.arrival_levels == r2.arrival_levels == [0.05, 0.5, 0.95]
    for r in (r1, r2):
        assert r.arrival.days == days and r.arrival.thresholds == [1.0, 10.0]
        assert r.arrival.total_weight == r.summary.total_weight > 0
        assert r.arrival.members == r.summary.members == r.evaluations - r.failed
    for k in range(2):
        for d in days + [None]:
            assert np.array_equal(r1.arrival.counts(k, d), r2.arrival.counts(k, d))
        for p in (0.05, 0.5, 0.95):
            assert np.array_equal(r1.arrival.quantile(k, p), r2.arrival.quantile(k, p))
        c1r, w1 = r1.arrival.reached(k)
        c2r, w2 = r2.arrival.reached(k)
        assert np.array_equal(c1r, c2r) and np.array_equal(w1, w2)
    assert np.array_equal(r1.arrival.prob_by(0, 0), r1.summary.exceedance(0, 0))
    npz_a, js_a = r1.save(str(tmp_path / 'a' / 'pp'))
    npz_p, js_p = plain.save(str(tmp_path / 'p' / 'pp'))
    labels = [str(one.days[d]) for d in days]
    with np.load(npz_p) as f:
        old = set(f.files)
    new = {'%s_parr%d_%s' % (lab, k, t) for lab in labels for k in (0, 1) for t in ('data', 'ind', 'indptr')}
    new |= {'arrival%d_%s' % (k, q) for k in (0, 1) for q in ('q5', 'q50', 'q95')}
    new |= {'arrival0_cells', 'arrival1_cells', 'arrival_weights'}
    N = 257
    with np.load(npz_a) as f:
        assert set(f.files) == old | new
        # the reference loader's rule (Plot_Result.py:515-524): `days`, then `{day}_*` CSR triplets
        assert [str(x) for x in f['days']] == labels
        for n, lab in enumerate(labels):
            M = sparse.csr_matrix((f[lab + '_data'], f[lab + '_ind'], f[lab + '_indptr']), shape=(N, N))
            m = r1.summary.mean(days[n])
            assert np.array_equal(M.toarray(), np.where(m >= 1e-8, m, 0.0))
            P = sparse.csr_matrix((f[lab + '_parr1_data'], f[lab + '_parr1_ind'], f[lab + '_parr1_indptr']),
                                  shape=(N, N))
            assert np.array_equal(P.toarray(), r1.arrival.prob_by(1, days[n]))
        q = f['arrival0_q50']
        assert q.dtype == np.int16 and np.array_equal(q, r1.arrival.quantile(0, 0.5))
        assert np.array_equal(f['arrival1_cells'], r1.arrival.reached(1)[0])
        assert np.array_equal(f['arrival_weights'], r1.arrival.reached(0)[1])
    import json
    meta = json.load(open(js_a))['predictive']['arrival']
    assert meta['thresholds'] == [1.0, 10.0] and meta['days'] == days and meta['levels'] == [0.05, 0.5, 0.95]
    assert meta['reached_area'] == [r1.arrival.reached_area(k, [0.05, 0.5, 0.95]) for k in range(2)]
    assert 'arrival' not in json.load(open(js_p))['predictive']
    for r in (r1, r2, plain):
        r.summary.close()
        if r.arrival is not None:
            r.arrival.close()
    for p in (one, pa, pb):
        p.close()
