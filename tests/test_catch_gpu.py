"""GPU tests of the catch-probability fields (ps_catch_*, predictive.CatchFields) and of the accumulators fed from
them: the device fields against mpmath and the numpy restatement (catch_ref), zeros, range and exact ones, gather,
determinism, the projection and release-plan sources, SpreadSummary / ReweightedSummary / MonteCarloError
.for_projection against the numpy loops fed the fetched bits, the untouched day-based path, the refusals, and
posterior_predictive(catch=) against a hand loop with its files.  Kalbar wind, 6 days, the members and weights of
test_projection_gpu.py."""
import ctypes as C
import json
import os
import types
import warnings

import numpy as np
import pytest

import catch_ref
import reweight_ref as RR
from test_arrival_gpu import MEMBERS, WEIGHTS, THR, _pop_model, _evaluate, _fields

pytestmark = pytest.mark.gpu

LEVELS = [0.5, 0.95]
ULP = 2.0 ** -52
# Device against restatement: the two differ in exp / expm1 alone, each library within 1 ulp of the exact
# exponential, so e differs by at most 2 ulp; the upper branch and n = 1 carry that to Y unchanged, the lower
# branch Y = 1 - e q with a factor e q / Y <= 0.55 / 0.45; one more ulp for the roundings that follow a changed e.
DEV_REF_RTOL = 4 * ULP


def _traps(fields):
    """nine traps over five of the six days, the inputs out of order and shared: rates from 1e-6 to 50, the middle
    ones put where the day's median density gives mu = n, so that both series run"""
    def mid(day, n):
        v = fields[day]
        return float(np.clip(n / np.median(v[v > 0]), 1e-6, 50.0))
    return [(1, 1e-6, 1), (3, 50.0, 5), (5, mid(5, 16), 16), (1, 50.0, 1), (3, mid(3, 2), 2), (5, 50.0, 16),
            (2, 1e-6, 5), (1, mid(1, 5), 5), (0, 1.0, 2)]


def _rel(got, ref):
    """|got - ref| / ref where ref >= 1e-290, else the absolute difference"""
    d = np.abs(got - ref)
    big = ref >= 1e-290
    out = d.copy()
    out[big] = d[big] / ref[big]
    return out


def _pick(mu, n, k=160):
    """indices of up to k + 44 non-zero entries of mu for mpmath: evenly through the sorted values, the ends, and
    the 20 on either side of mu = n"""
    nz = np.flatnonzero(mu > 0)
    order = nz[np.argsort(mu[nz])]
    at = int(np.searchsorted(mu[order], float(n)))
    take = set(order[np.linspace(0, order.size - 1, min(k, order.size)).astype(int)])
    take |= set(order[max(at - 20, 0):at + 20]) | {order[0], order[-1]}
    return np.array(sorted(take))


def _check_fields(CF, v_of_output, seen):
    """every output of CF against v (its input's value field): zeros, range, the restatement everywhere and mpmath
    on a sample; seen: counters of the cases the data hit"""
    worst_ref = worst_dev = worst_full = 0.0
    for e, (key, rate, n) in enumerate(CF.traps):
        v = v_of_output[e]
        Y = CF.field(e)
        assert Y.dtype == np.float64 and Y.shape == v.shape
        assert np.array_equal(Y == 0.0, v == 0.0) and not np.signbit(Y).any(), e
        assert ((Y >= 0.0) & (Y <= 1.0)).all(), e
        mu = (np.float64(rate) * v).ravel()
        ref = catch_ref.catch_value(mu, n)
        full = _rel(Y.ravel(), ref)
        worst_full = max(worst_full, full.max())
        idx = _pick(mu, n)
        err_ref = catch_ref.rel_errors(ref[idx], mu[idx], n)
        err_dev = catch_ref.rel_errors(Y.ravel()[idx], mu[idx], n)
        worst_ref, worst_dev = max(worst_ref, err_ref.max()), max(worst_dev, err_dev.max())
        seen['upper'] += int(((mu > 0) & (mu < n)).sum())
        seen['lower'] += int((mu >= n).sum())
        seen['zero'] += int((mu == 0).sum())
        seen['one'] += int((Y == 1.0).sum())
    print('largest error against mpmath: device %.3g, restatement %.3g; device against restatement %.3g'
          % (worst_dev, worst_ref, worst_full))
    return worst_dev, worst_ref, worst_full


@pytest.mark.parametrize('R', [64, 128])
def test_fields_against_mpmath_and_the_restatement(R):
    from parasitoids_amd.predictive import CatchFields
    pm = _pop_model(R)
    N = 2 * R + 1
    _evaluate(pm, MEMBERS[0])
    fields = _fields(pm, range(6))
    traps = _traps(fields)
    assert min(t[1] for t in traps) == 1e-6 and max(t[1] for t in traps) == 50.0
    assert {t[2] for t in traps} == {1, 2, 5, 16}
    with CatchFields(pm, traps) as CF:
        assert CF.in_days == [0, 1, 2, 3, 5] and CF.nout == 9 and CF.fields_kind == 'catch'
        assert CF.nbytes == 9 * ((N * N + 63) // 64 * 64) * 8
        CF.apply()
        assert CF.applies == 1
        seen = dict(upper=0, lower=0, zero=0, one=0)
        dev, ref, full = _check_fields(CF, [fields[t[0]] for t in traps], seen)
        print('cells: %r' % (seen,))
        assert all(c > 0 for c in seen.values()), seen
        assert dev <= 4 * ref
        assert full <= DEV_REF_RTOL
        # gather: the tail cell of the odd N * N, its neighbour, the release cell and a corner
        rows, cols = [N - 1, N - 1, R, 0, R + 1], [N - 1, N - 2, R, 0, R - 2]
        got = CF.gather(rows, cols)
        assert got.shape == (9, 5)
        for e in range(9):
            assert np.array_equal(got[e], CF.field(e)[rows, cols])
        assert got[:, 2].min() > 0               # the release cell holds wasps on every day
    pm.close()


def test_determinism_overwrite_and_the_other_sources():
    from parasitoids_amd.predictive import CatchFields, Projection, ReleaseSites
    pm = _pop_model(64, mode='exact')
    res_m = 10000.0 / 64
    _evaluate(pm, MEMBERS[0])
    fields = _fields(pm, range(6))
    traps = _traps(fields)
    days = [0, 1, 2, 3, 5]
    by_index = [(days.index(d), r, n) for d, r, n in traps]
    plan_days = [0, 1, 3, 5]
    plan_traps = [t for t in traps if t[0] in plan_days]
    with CatchFields(pm, traps) as CF, Projection(pm, np.eye(5), days) as P, \
            CatchFields.for_projection(P, by_index) as CP, \
            ReleaseSites(pm, [(0.0, 0.0, 0.6), (7 * res_m, -3 * res_m, 0.5)], plan_days) as RS, \
            CatchFields.for_projection(RS, plan_traps) as CS:
        CF.apply()
        first = [CF.field(e) for e in range(9)]
        CF.apply()
        assert all(np.array_equal(CF.field(e), first[e]) for e in range(9))
        # identity weights: the projection's outputs are the day fields, and so are the catch fields, bit for bit
        P.apply()
        CP.apply()
        assert all(np.array_equal(CP.field(e), first[e]) for e in range(9))
        # a release plan: the restatement applied to the plan's fetched fields
        RS.apply()
        CS.apply()
        plan = {d: RS.field(e) for e, d in enumerate(plan_days)}
        seen = dict(upper=0, lower=0, zero=0, one=0)
        dev, ref, full = _check_fields(CS, [plan[t[0]] for t in plan_traps], seen)
        assert dev <= 4 * ref and full <= DEV_REF_RTOL and seen['upper'] > 0 and seen['zero'] > 0
        # a second member overwrites the first, zeros included
        _evaluate(pm, MEMBERS[2])
        CF.apply()
        other = _fields(pm, range(6))
        second = [CF.field(e) for e in range(9)]
        assert any(not np.array_equal(a, b) for a, b in zip(first, second))
        assert any(((a == 0) != (b == 0)).any() for a, b in zip(first, second))   # another zero pattern, checked below
        dev, ref, full = _check_fields(CF, [other[t[0]] for t in traps], dict(upper=0, lower=0, zero=0, one=0))
        assert dev <= 4 * ref and full <= DEV_REF_RTOL
        assert CF.applies == 3 and CP.applies == 1
        # output labels that do not exist, or carry no weight, are refused on the host
        with pytest.raises(ValueError, match='output'):
            CatchFields.for_projection(RS, [(2, 1.0)])
        with pytest.raises(ValueError, match='output'):
            CatchFields.for_projection(P, [(5, 1.0)])
    pm.close()


@pytest.fixture(scope='module')
def fed():
    """the five members in three passes on one exact-mode model (the same member gives the same bits each time):
    first every accumulator fed without a host synchronisation in between, then the members in another order with
    their catch fields fetched, then a day summary alone"""
    from parasitoids_amd.predictive import (CatchFields, MonteCarloError, ReweightedSummary, SpreadSummary)
    f = types.SimpleNamespace()
    pm = f.pm = _pop_model(64, mode='exact')
    _evaluate(pm, MEMBERS[0])
    f.traps = _traps(_fields(pm, range(6)))
    f.CF = CatchFields(pm, f.traps)
    f.S = SpreadSummary.for_projection(f.CF, LEVELS)
    f.Sa, f.Sb = SpreadSummary.for_projection(f.CF, LEVELS), SpreadSummary.for_projection(f.CF, LEVELS)
    f.S2 = SpreadSummary.for_projection(f.CF, LEVELS)
    f.RW = ReweightedSummary.for_projection(f.CF, ['flat'], LEVELS)
    f.M = MonteCarloError.for_projection(f.CF, 3, LEVELS)
    f.D_with, f.D_alone = SpreadSummary(pm, None, THR), SpreadSummary(pm, None, THR)
    for m, w in zip(MEMBERS, WEIGHTS):                       # nothing here waits for the device
        _evaluate(pm, m)
        f.D_with.add(w)
        f.CF.apply()
        f.S.add(w)
        f.RW.add([0.0], w)
        f.M.add(w)
        (f.Sa if m in MEMBERS[:2] else f.Sb).add(w)
    f.M.finish()
    f.Y = [None] * 5
    f.order = [3, 0, 4, 1, 2]
    for i in f.order:
        _evaluate(pm, MEMBERS[i])
        f.CF.apply()
        f.S2.add(WEIGHTS[i])
        f.Y[i] = np.array([f.CF.field(e) for e in range(len(f.traps))])
    for m, w in zip(MEMBERS, WEIGHTS):
        _evaluate(pm, m)
        f.D_alone.add(w)
    yield f
    for h in (f.S, f.Sa, f.Sb, f.S2, f.RW, f.M, f.D_with, f.D_alone, f.CF):
        h.close()
    pm.close()


def test_summary_of_catch_fields_against_the_numpy_loop(fed):
    S, n = fed.S, len(fed.traps)
    assert (S.total_weight, S.members, S.thresholds) == (8.0, 5, LEVELS)
    st = RR.new_state(fed.Y[0].shape, LEVELS, 1)
    for i in range(5):
        RR.add(st, fed.Y[i], [0.0], WEIGHTS[i])
    sc = st[0]
    for e in range(n):
        assert np.array_equal(S.mean(e), sc['mean'][e]), e                      # bit for bit
        for k in range(2):
            assert np.array_equal(S.exceedance(e, k), RR.exceedance(sc, k)[e]), (e, k)   # the counts, exactly
        scale = np.abs(sc['mean'][e]).max()
        np.testing.assert_allclose(S.variance(e), RR.variance(sc)[e], rtol=1e-12, atol=1e-15 * scale ** 2)
        assert (S.mean(e) <= 1.0).all() and S.mean(e).max() > 0
    # the members' fields do differ, and some cell is surely caught in: the summary is not trivial
    assert any(S.variance(e).max() > 0 for e in range(n))
    assert any((S.exceedance(e, 1) == 1.0).any() for e in range(n))


def test_add_order_and_two_way_merge(fed):
    S, n = fed.S, len(fed.traps)
    fed.Sa.merge(fed.Sb)
    for other in (fed.S2, fed.Sa):
        assert (other.total_weight, other.members) == (8.0, 5)
        for e in range(n):
            m = S.mean(e)
            scale = np.abs(m).max()
            np.testing.assert_allclose(other.mean(e), m, rtol=1e-12, atol=1e-15 * scale)
            np.testing.assert_allclose(other.variance(e), S.variance(e), rtol=1e-12, atol=1e-15 * scale ** 2)
            for k in range(2):
                assert np.array_equal(other.exceedance(e, k), S.exceedance(e, k))


def test_reweighted_summary_with_zero_log_weights_holds_the_summary_bits(fed):
    S, RW = fed.S, fed.RW
    assert RW.members('flat') == 5 and RW.skipped('flat') == 0
    for e in range(len(fed.traps)):
        assert np.array_equal(RW.mean('flat', e), S.mean(e))
        assert np.array_equal(RW.variance('flat', e), S.variance(e))
        for k in range(2):
            assert np.array_equal(RW.exceedance('flat', e, k), S.exceedance(e, k))


def test_monte_carlo_error_of_catch_fields_against_the_replay(fed):
    from test_mcerr_gpu import _check_exact, _replay
    n = len(fed.traps)
    ref = _replay(fed.Y, WEIGHTS, LEVELS, 3)
    assert (fed.M.batches, fed.M.used_weight, fed.M.discarded_weight) == (2, 6, 2)
    _check_exact(fed.M, ref, list(range(n)))


def test_the_day_summary_beside_a_catch_handle_does_not_move(fed):
    A, B = fed.D_with, fed.D_alone
    assert A.total_weight == B.total_weight == 8.0
    for d in A.days:
        assert np.array_equal(A.mean(d), B.mean(d)) and np.array_equal(A.variance(d), B.variance(d))
        for k in range(2):
            assert np.array_equal(A.exceedance(d, k), B.exceedance(d, k))


def test_refusals():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import CatchFields, Projection, SpreadSummary
    lib = L.load()
    N = 129

    def create(nin, nout, inputs, rates, counts, n=N):
        h = L._VP()
        rc = lib.ps_catch_create(0, n, nin, nout, L.p_i32(L.i32(inputs)), L.p_f64(L.f64(rates)),
                                 L.p_i32(L.i32(counts)), C.byref(h))
        if rc == L.PS_OK:
            lib.ps_catch_destroy(h)
        return rc
    assert create(2, 2, [0, 1], [1.0, 2.0], [1, 16]) == L.PS_OK
    for args in [(0, 1, [0], [1.0], [1]), (33, 1, [0], [1.0], [1]), (1, 0, [0], [1.0], [1]),
                 (1, 33, [0] * 33, [1.0] * 33, [1] * 33), (2, 1, [2], [1.0], [1]), (2, 1, [-1], [1.0], [1]),
                 (1, 1, [0], [0.0], [1]), (1, 1, [0], [-1.0], [1]), (1, 1, [0], [float('inf')], [1]),
                 (1, 1, [0], [float('nan')], [1]), (1, 1, [0], [1.0], [0]), (1, 1, [0], [1.0], [17]),
                 (2, 2, [0, 1], [1.0, 0.0], [1, 1])]:
        assert create(*args) == L.PS_ERR_BAD_ARG, args
    assert create(1, 1, [0], [1.0], [1], n=0) == L.PS_ERR_BAD_ARG
    with pytest.raises(ValueError, match='count'):
        CatchFields(types.SimpleNamespace(), [(1, 1.0, 2.5)])        # refused before the model is looked at
    pm = _pop_model(64)
    with CatchFields(pm, [(1, 1.0), (2, 0.5, 3)]) as CF, SpreadSummary.for_projection(CF, LEVELS) as S, \
            Projection(pm, np.eye(3), [0, 1, 2]) as P3, SpreadSummary.for_projection(P3, LEVELS) as S3:
        # before the model's first evaluation: as Projection.apply
        with pytest.raises(ValueError, match='evaluation'):
            CF.apply()
        with pytest.raises(ValueError, match='evaluation'):
            P3.apply()
        _evaluate(pm, MEMBERS[0])
        # before the first apply
        for call in (lambda: CF.field(0), lambda: CF.gather([0], [0]), lambda: S.add(1)):
            with pytest.raises(L.HipError) as ei:
                call()
            assert ei.value.code == L.PS_ERR_STATE
        CF.apply()
        # slot counts and domains that do not fit: nothing is enqueued, the accumulator stays empty
        assert lib.ps_summary_add_catch(S3._h, CF._h, 1) == L.PS_ERR_BAD_ARG
        assert S3.members == 0
        other = L._VP()
        thr = L.f64(LEVELS)
        L.check(lib.ps_summary_create(0, 131, 2, 2, L.p_f64(thr), C.byref(other)))
        assert lib.ps_summary_add_catch(other, CF._h, 1) == L.PS_ERR_BAD_ARG
        lib.ps_summary_destroy(other)
        assert lib.ps_summary_add_catch(S._h, CF._h, 0) == L.PS_ERR_BAD_ARG       # weight >= 1
        assert lib.ps_summary_add_catch(S._h, None, 1) == L.PS_ERR_BAD_ARG
        # a source with another number of outputs than the handle has inputs
        assert lib.ps_catch_apply_project(CF._h, P3._h) == L.PS_ERR_STATE          # P3 not applied yet
        P3.apply()
        assert lib.ps_catch_apply_project(CF._h, P3._h) == L.PS_ERR_BAD_ARG        # 3 outputs, 2 inputs
        assert CF.applies == 1
        with pytest.raises(ValueError):
            CF.field(2)
        with pytest.raises(L.HipError):
            CF.gather([129], [0])
        S.add(2)
        assert S.members == 1 and S.total_weight == 2.0
    # the other two accumulators: state and slot count
    from parasitoids_amd.predictive import MonteCarloError, ReweightedSummary
    with CatchFields(pm, [(1, 1.0), (2, 0.5, 3)]) as CF, MonteCarloError.for_projection(CF, 2, LEVELS) as M, \
            ReweightedSummary.for_projection(CF, ['a'], LEVELS) as RW, CatchFields(pm, [(1, 1.0)]) as C1:
        for call in (lambda: M.add(1), lambda: RW.add([0.0], 1)):
            with pytest.raises(L.HipError) as ei:
                call()
            assert ei.value.code == L.PS_ERR_STATE
        C1.apply()
        one = L.f64([1.0])
        assert lib.ps_mcerr_add_catch(M._h, C1._h, 1) == L.PS_ERR_BAD_ARG
        assert lib.ps_wsum_add_catch(RW._h, C1._h, 1, L.p_f64(one), L.p_f64(one)) == L.PS_ERR_BAD_ARG
        assert M.members == 0 and RW.members('a') == 0
    pm.close()


def _csr(f, key, N):
    from scipy import sparse
    return sparse.csr_matrix((f[key + '_data'], f[key + '_ind'], f[key + '_indptr']), shape=(N, N)).toarray()


def test_posterior_predictive_with_catch_against_a_hand_loop(tmp_path):
    from parasitoids_amd import mcmc
    from parasitoids_amd import predictive as PR
    from test_reweight_gpu import _chain
    R, N = 64, 129
    res_m = 10000.0 / R
    ta, names = _chain([3, 2])
    tb, _ = _chain([1, 2, 2])
    traces = [ta, tb[1:]]                                    # the second chain: two runs of other members
    chains = [(t, names) for t in traces]
    traps = [(1, 0.01), (1, 1.0), (1, 50.0), (3, 1.0, 2), (5, 5.0, 16)]
    em = dict(collection_day=6, obs_days=[19, 21, 24])
    em_traps = [(19, 0.5), (24, 2.0, 3)]
    plan = dict(sites=[(0.0, 0.0, 0.6), (7 * res_m, -3 * res_m, 0.5)], days=[0, 1, 3, 5])
    arg = dict(traps=traps, levels=LEVELS, emergence=em_traps)
    rw = {'flat': dict(log_weights=[np.zeros(len(t)) for t in traces]), 'options': dict(min_ess=1)}
    pm = _pop_model(R, mode='exact')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        res = PR.posterior_predictive(pm, chains, thresholds=THR, catch=arg, emergence=em, sites=plan, reweight=rw,
                                      mc_error=dict(batches=4), cell_area=res_m ** 2)
    cp = res.catch
    assert res.failed == 0 and res.evaluations == 4
    assert cp.traps == [(1, 0.01, 1), (1, 1.0, 1), (1, 50.0, 1), (3, 1.0, 2), (5, 5.0, 16)] and cp.levels == LEVELS
    assert (cp.summary.total_weight, cp.summary.members) == (9.0, 4)
    # the hand loop: every run once more, per chain a summary of its own, merged in chain order
    cols = [names.index(m[0]) for m in mcmc.MODEL_BLOCK]
    W, in_days, labels = PR.emergence_plan(em, 6)
    hand, hand_em, hand_pl = [], [], []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        with PR.CatchFields(pm, traps) as CF, PR.Projection(pm, W, in_days) as P, \
                PR.CatchFields.for_projection(P, em_traps, labels) as CE, \
                PR.ReleaseSites(pm, plan['sites'], plan['days']) as RS, \
                PR.CatchFields.for_projection(RS, traps) as CS:
            for ci in range(2):
                hand.append(PR.SpreadSummary.for_projection(CF, LEVELS))
                hand_em.append(PR.SpreadSummary.for_projection(CE, LEVELS))
                hand_pl.append(PR.SpreadSummary.for_projection(CS, LEVELS))
                for c, first, weight in res.runs:
                    if c != ci:
                        continue
                    pm.evaluate(*mcmc.model_args(traces[ci][first, cols]), want_stats=False)
                    CF.apply()
                    hand[ci].add(weight)
                    P.apply()
                    CE.apply()
                    hand_em[ci].add(weight)
                    RS.apply()
                    CS.apply()
                    hand_pl[ci].add(weight)
            for hs in (hand, hand_em, hand_pl):
                hs[0].merge(hs[1])
                hs[1].close()
    for got, want, n in ((cp, hand[0], 5), (res.emergence.catch, hand_em[0], 2), (res.sites.catch, hand_pl[0], 5)):
        assert got.summary.total_weight == want.total_weight == 9.0
        for e in range(n):
            assert np.array_equal(got.prob(e), want.mean(e)), e
            var = want.variance(e)
            assert np.array_equal(got.summary.variance(e), var), e
            assert np.array_equal(got.sd(e), np.sqrt(np.maximum(var, 0.0))), e
            for k in range(2):
                assert np.array_equal(got.sure(e, k), want.exceedance(e, k)), (e, k)
    assert res.emergence.catch.traps == [(19, 0.5, 1), (24, 2.0, 3)]
    # more effort catches more, a higher count less; the ladder of day 1 as a step function
    assert (cp.prob(0) <= cp.prob(1) + 1e-15).all() and (cp.prob(1) <= cp.prob(2) + 1e-15).all()
    assert cp.prob(2).max() > 0.95
    need = cp.required_rate(1, 1, 0.95)
    assert np.array_equal(need, PR.required_rate(cp.traps, [cp.prob(e) for e in range(5)], 1, 1, 0.95), equal_nan=True)
    assert set(np.unique(need[~np.isnan(need)])) <= {0.01, 1.0, 50.0} and np.isnan(need).any() and (need == 50.0).any()
    # log-weights 0: the reweighted catch maps hold the summary's bits; the Monte Carlo error has its own handle
    for got in (cp, res.emergence.catch, res.sites.catch):
        assert np.array_equal(got.reweight.mean('flat', 0), got.prob(0))
        assert (got.mc_error.batches, got.mc_error.used_weight) == (res.mc_error.batches, res.mc_error.used_weight)
        assert got.mc_error.batches >= 4 and got.mc_error.thresholds == LEVELS
        assert np.isfinite(got.mc_error.mcse(0)).all()
    # the files
    npz, js = res.save(str(tmp_path / 'a' / 'pp'))
    names_out = sorted(os.listdir(str(tmp_path / 'a')))
    for want in ('pp_catch.npz', 'pp_emergence_catch.npz', 'pp_sites_catch.npz', 'pp_catch_reweight.npz'):
        assert want in names_out
    f = np.load(str(tmp_path / 'a' / 'pp_catch.npz'))
    assert list(f['days']) == [1, 1, 1, 3, 5] and list(f['rates']) == [0.01, 1.0, 50.0, 1.0, 5.0]
    assert list(f['counts']) == [1, 1, 1, 2, 16] and list(f['levels']) == LEVELS
    for e in range(5):
        for key, m in (('c%d' % e, cp.prob(e)), ('c%d_sd' % e, cp.sd(e)), ('c%d_sure1' % e, cp.sure(e, 1))):
            assert np.array_equal(_csr(f, key, N), np.where(m >= 1e-8, m, 0.0)), key
    fe = np.load(str(tmp_path / 'a' / 'pp_emergence_catch.npz'))
    assert list(fe['days']) == [19, 24] and 'c1_sure0_data' in fe.files
    meta = json.load(open(js))['predictive']
    block = meta['catch']
    assert block['given'] == {'traps': [list(t) for t in traps], 'levels': LEVELS,
                              'emergence': [list(t) for t in em_traps]}
    assert block['members'] == 4 and block['total_weight'] == 9.0 and block['levels'] == LEVELS
    for e, out in enumerate(block['outputs']):
        m = cp.prob(e)
        assert out['trap'] == list(cp.traps[e]) and out['max_prob'] == float(m.max())
        assert out['area'] == [float((m >= p).sum() * res_m ** 2) for p in LEVELS]
    assert meta['emergence']['catch']['traps'] == [[19, 0.5, 1], [24, 2.0, 3]]
    assert len(meta['sites']['catch']['outputs']) == 5
    assert 'catch' in meta['mc_error'] and 'sites_catch' in meta['mc_error']
    for h in (hand[0], hand_em[0], hand_pl[0], res.summary, res.reweight, res.mc_error, res.emergence, res.sites, cp):
        h.close()
    # a trap day the plan does not output is refused before any evaluation
    with pytest.raises(ValueError, match='output day'):
        PR.posterior_predictive(pm, chains, catch=dict(traps=[(2, 1.0)]), sites=plan)
    pm.close()


def test_without_catch_nothing_changes(tmp_path):
    from parasitoids_amd import predictive as PR
    from test_reweight_gpu import _chain
    pm = _pop_model(64)
    trace, names = _chain([2, 1])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        res = PR.posterior_predictive(pm, (trace, names), thresholds=THR, emergence=dict(collection_day=6))
    assert res.catch is None and res.emergence.catch is None
    res.save(str(tmp_path / 'p' / 'pp'))
    assert sorted(os.listdir(str(tmp_path / 'p'))) == ['pp.json', 'pp.npz', 'pp_emergence.npz']
    meta = json.load(open(str(tmp_path / 'p' / 'pp.json')))['predictive']
    assert 'catch' not in meta and 'catch' not in meta['emergence']
    res.summary.close()
    res.emergence.close()
    pm.close()
