"""GPU tests of the ranking of several named plans (ps_rank_*, predictive.PlanRanking): the device's regret means,
count planes and coverage rows bit for bit against the numpy replay (rank_ref) of the plans' fetched fields, the
variances within the tolerances of the contrast tests; two plans against PlanContrast, a permutation of the plans,
a twin plan, exact scaling, weights, merges and reset, the untouched accumulators beside it, a tuple of three
projections, posterior_predictive with ranking=, the refusals of the C ABI, and the grid-stride path at R = 768.
Kalbar wind, R = 64 (N = 129: odd, so the tail cell and the pairs that straddle a row end exist), 6 days, the
members, weights and plans of test_sites_gpu.py.  Plan C is one site of amount 1.5 at the centre and a copy of plan
B's site at the north edge: with the centre site alone no cell holds a positive tie (the fields of different sites
never agree to the last bit), and the tie branch of the kernel would go untested; around the shared site B and C
hold the same value exactly and A holds nothing."""
import ctypes as C
import json
import os
import types
import warnings

import numpy as np
import pytest

import rank_ref
from test_sites_gpu import MEMBERS, STAGGERED, WEIGHTS, _chain, _csr, _edge_plan, _evaluate, _metres, _pop_model

pytestmark = pytest.mark.gpu

R, N = 64, 129
THR = [1.0, 10.0]
DAYS = list(range(6))
OUT = [0, 1, 2, 3, 5]
PLAN_A = STAGGERED                                                       # a group released two days later
PLAN_B = [(dr, dc, 0.75 * a, lag) for dr, dc, a, lag in _edge_plan(R)]     # scaled: either side wins somewhere
PLAN_C = [(0, 0, 1.5, 0), PLAN_B[5]]                                     # the centre, and B's site at the north edge


def _double(plan):
    return [(dr, dc, 2.0 * a, lag) for dr, dc, a, lag in plan]


def _replay(fields, weights, thr, members=None, order=None):
    """per output the rank_ref state over the members' fields [member][output][plan] (order: the plans taken)"""
    idx = range(len(weights)) if members is None else members
    states = []
    for e in range(len(fields[0])):
        nplan = len(fields[0][e]) if order is None else len(order)
        st = rank_ref.new_state(fields[0][e][0].shape, nplan, thr)
        for i in idx:
            rank_ref.add(st, fields[i][e] if order is None else [fields[i][e][j] for j in order], weights[i])
        states.append(st)
    return states


def _check_exact(K, states, nout):
    """every regret mean, every count plane and every coverage row of K against the replay, bit for bit"""
    nthr = len(K.thresholds)
    for e in range(nout):
        st = states[e]
        for j in range(K.nplan):
            got = K.regret(e, j)
            assert np.array_equal(got, st['mean'][j]), (e, j, np.abs(got - st['mean'][j]).max())
        planes = rank_ref.planes(st)
        assert len(planes) == K.nplanes
        for which, plane in enumerate(planes):
            got = K.counts(e, which)
            assert got.dtype == np.uint32 and np.array_equal(got.astype(np.int64), plane), (e, which)
    for k in range(nthr):
        cells, w = K.coverage(k)
        assert cells.dtype == np.int64 and cells.shape == (len(states[0]['weights']), K.nplan, nout)
        assert list(w) == states[0]['weights']
        for e in range(nout):
            assert np.array_equal(cells[:, :, e], rank_ref.rows(states[e])[:, :, k]), (k, e)


def _check_variance(K, fields, weights, nout):
    """against a numpy two-pass, the tolerances of test_contrast_gpu._check_variance: rtol 1e-12, atol 1e-15 scale^2"""
    for e in range(nout):
        reg = rank_ref.regrets([m[e] for m in fields])
        for j in range(K.nplan):
            _mean, var = rank_ref.two_pass(reg[:, j], weights)
            scale = np.abs(reg[:, j]).max()
            got = K.regret_variance(e, j)
            print('variance, output %d plan %d: max abs error %.3g, scale^2 %.3g' % (e, j, np.abs(got - var).max(), scale ** 2))
            np.testing.assert_allclose(got, var, rtol=1e-12, atol=1e-12 * 1e-3 * scale ** 2)


def _same_counts(K, other, nout, planes=None):
    for e in range(nout):
        for which in (range(K.nplanes) if planes is None else planes):
            assert np.array_equal(K.counts(e, which), other.counts(e, which)), (e, which)


@pytest.fixture(scope='module')
def fed():
    """the plans A (staggered), B (the edge plan), C, a twin of A and all three doubled, applied to the five members,
    every accumulator the tests read fed alongside, the fields fetched, and the replay computed once"""
    from parasitoids_amd.predictive import (ArrivalMaps, PlanContrast, PlanRanking, ReleaseSites, SpreadHistogram,
                                            SpreadSummary, lagged_models)
    pm = _pop_model(R)
    late = lagged_models(pm, [2])
    f = types.SimpleNamespace(pm=pm, late=late)
    f.A = A = ReleaseSites(pm, _metres(PLAN_A, R), OUT, late)
    f.A2 = A2 = ReleaseSites(pm, _metres(PLAN_A, R), OUT, late)
    f.B = B = ReleaseSites(pm, _metres(PLAN_B, R), OUT)
    f.C = Cp = ReleaseSites(pm, _metres(PLAN_C, R), OUT)
    f.doubled = [ReleaseSites(pm, _metres(_double(PLAN_A), R), OUT, late), ReleaseSites(pm, _metres(_double(PLAN_B), R), OUT),
                 ReleaseSites(pm, _metres(_double(PLAN_C), R), OUT)]
    f.K = PlanRanking([A, B, Cp], THR, ['a', 'b', 'c'])
    f.Kperm = PlanRanking([Cp, A, B], THR)
    f.Ktwin = PlanRanking([A, A2, B], THR)
    f.K2 = PlanRanking([A, B], THR)
    f.Kdouble = PlanRanking(f.doubled, [2.0 * t for t in THR])
    f.K0 = PlanRanking([A, B, Cp])                           # no thresholds: best and regret alone, no rows
    f.Kunit = PlanRanking([A, B, Cp], THR)
    f.Klo, f.Khi = PlanRanking([A, B, Cp], THR), PlanRanking([A, B, Cp], THR)
    f.X, f.Xba = PlanContrast(A, B, THR), PlanContrast(B, A, THR)
    f.S, f.SB = SpreadSummary.for_projection(A, THR), SpreadSummary.for_projection(B, THR)
    f.H, f.Arr = SpreadHistogram.for_projection(A), ArrivalMaps.for_projection(A, THR)
    f.rankings = [f.K, f.Kperm, f.Ktwin, f.K2, f.Kdouble, f.K0, f.Kunit, f.Klo, f.Khi]
    f.fields = []
    for i, (mem, w) in enumerate(zip(MEMBERS, WEIGHTS)):
        _evaluate(pm, mem)
        _evaluate(late[2], mem, ndays=4)
        A.apply()
        for acc in (f.S, f.H, f.Arr):
            acc.add(w)
        for plan in [B, Cp, A2] + f.doubled:
            plan.apply()
        f.SB.add(w)
        for acc in (f.K, f.Kperm, f.Ktwin, f.K2, f.Kdouble, f.K0, f.X, f.Xba, f.Klo if i < 2 else f.Khi):
            acc.add(w)
        for _ in range(w):
            f.Kunit.add(1)
        f.fields.append([[A.field(e), B.field(e), Cp.field(e)] for e in range(len(OUT))])
    f.ref = _replay(f.fields, WEIGHTS, THR)
    yield f
    for h in f.rankings + [f.X, f.Xba, f.S, f.SB, f.H, f.Arr, A, A2, B, Cp] + f.doubled + [pm, late[2]]:
        h.close()


def test_against_the_reference_bit_for_bit(fed):
    from parasitoids_amd.predictive import coverage_ranking
    K, ref = fed.K, fed.ref
    pitch = (N * N + 63) // 64 * 64
    assert K.N == N and K.nout == 5 and K.labels == OUT and K.live == list(range(5)) and K.thresholds == THR
    assert K.nplan == 3 and K.names == ['a', 'b', 'c'] and K.nplanes == 3 + 2 * 5
    assert K.total_weight == sum(WEIGHTS) and K.members == len(MEMBERS)
    assert K.nbytes == 5 * pitch * (16 * 3 + 4 * 13) and K.cell_area == (10000.0 / R) ** 2
    # the inputs can fail: every plan sole best somewhere, a positive tie, every sole / any / all plane non-zero for
    # some output, all != any, something in the last row or column, coverage rows that tell the plans apart
    a = np.array(fed.fields)                                 # [member, output, plan, N, N]
    top = a.max(axis=2)
    holders = (a == top[:, :, None]).sum(axis=2)
    for j in range(3):
        assert max(st['best'][j].max() for st in ref) > 0, j
    assert ((holders > 1) & (top > 0)).any()
    for k in range(len(THR)):
        for j in range(3):
            assert max(st['sole'][k, j].max() for st in ref) > 0, (k, j)
        assert max(st['any'][k].max() for st in ref) > 0 and max(st['all'][k].max() for st in ref) > 0
        assert any((st['all'][k] != st['any'][k]).any() for st in ref)
    assert a[..., N - 1, :].any() or a[..., :, N - 1].any()
    assert all(len({tuple(r) for r in rank_ref.rows(st)[0].tolist()}) == 3 for st in ref)
    _check_exact(K, ref, 5)
    _check_variance(K, fed.fields, WEIGHTS, 5)
    W = float(sum(WEIGHTS))
    for e, j, k in ((2, 0, 0), (4, 2, 1), (0, 1, 1)):
        st = ref[e]
        assert np.array_equal(K.prob_best(e, j), st['best'][j] / W)
        assert np.array_equal(K.sole(e, k, j), st['sole'][k, j] / W)
        assert np.array_equal(K.any(e, k), st['any'][k] / W) and np.array_equal(K.all(e, k), st['all'][k] / W)
        assert np.array_equal(K.regret_sd(e, j), np.sqrt(K.regret_variance(e, j)))
        assert np.array_equal(K.prob_undecided(e), 1.0 - st['best'].sum(axis=0) / W)
        lead = K.leader(e)
        want = np.where(st['best'].max(axis=0) > 0, np.argmax(st['best'], axis=0), -1)
        assert lead.dtype == np.int8 and np.array_equal(lead, want)
    assert set().union(*[{int(v) for v in np.unique(K.leader(e))} for e in range(5)]) == {-1, 0, 1, 2}
    assert list(K.weights) == WEIGHTS
    # without thresholds: the same moments and best planes, no threshold planes and no rows
    K0 = fed.K0
    assert K0.nbytes == 5 * pitch * (16 * 3 + 4 * 3) and K0.nplanes == 3 and list(K0.weights) == WEIGHTS
    for e in range(5):
        for j in range(3):
            assert np.array_equal(K0.regret(e, j), K.regret(e, j))
            assert np.array_equal(K0.regret_variance(e, j), K.regret_variance(e, j))
            assert np.array_equal(K0.counts(e, j), K.counts(e, j))
    with pytest.raises(ValueError):
        K0.counts(0, 3)
    with pytest.raises(ValueError):
        K0.coverage(0)
    with pytest.raises(ValueError):
        K.regret(0, 3)
    rank = K.coverage_ranking(1, (0.5,))
    cells, w = K.coverage(1)
    assert [r['label'] for r in rank] == OUT and [p['name'] for p in rank[0]['plans']] == ['a', 'b', 'c']
    plain = coverage_ranking(cells, w, K.cell_area, (0.5,))
    for r, p in zip(rank, plain):
        assert r['p_tied'] == p['p_tied']
        assert [{k: v for k, v in x.items() if k != 'name'} for x in r['plans']] == p['plans']


def test_two_plans_are_the_contrast(fed):
    K2, X = fed.K2, fed.X
    W = fed.S.total_weight
    assert K2.nplanes == 2 + 2 * 4
    assert max(X.counts(e, 0).max() for e in range(5)) > 0 and max(X.counts(e, 1).max() for e in range(5)) > 0
    differ = 0
    for e in range(5):
        assert np.array_equal(K2.counts(e, 0), X.counts(e, 0)) and np.array_equal(K2.counts(e, 1), X.counts(e, 1))
        for k in range(2):
            assert np.array_equal(K2.counts(e, 2 + 4 * k), X.counts(e, 2 + 2 * k))          # sole_k0 = gain_k
            assert np.array_equal(K2.counts(e, 3 + 4 * k), X.counts(e, 3 + 2 * k))          # sole_k1 = loss_k
            na = np.rint(fed.S.exceedance(e, k) * W).astype(np.int64)
            nb = np.rint(fed.SB.exceedance(e, k) * W).astype(np.int64)
            some = K2.counts(e, 4 + 4 * k).astype(np.int64)
            every = K2.counts(e, 5 + 4 * k).astype(np.int64)
            assert np.array_equal(some, na + nb - every)
            differ += int(every.max() > 0 and (some != every).any())
        # the regret of A is the positive part of B - A, that of B the positive part of A - B: their means differ by
        # the contrast's mean up to the rounding of three running means over five members (three rounded operations
        # a step, each below an ulp of the largest |d|: under 50 ulp in all)
        d = X.mean(e)
        np.testing.assert_allclose(K2.regret(e, 1) - K2.regret(e, 0), d, rtol=1e-12, atol=1e-14 * np.abs(d).max())
    assert differ > 0
    for k in range(2):
        cells, w = K2.coverage(k)
        ca, cb, cw = X.coverage(k)
        assert np.array_equal(cells[:, 0], ca) and np.array_equal(cells[:, 1], cb) and np.array_equal(w, cw)
        rank, diff = K2.coverage_ranking(k), X.coverage_difference(k)
        for r, d in zip(rank, diff):
            assert r['plans'][0]['p_most'] == d['p_a_larger'] and r['plans'][1]['p_most'] == d['p_b_larger']


def test_a_permutation_of_the_plans_permutes_the_planes(fed):
    K, Kp = fed.K, fed.Kperm
    perm = [2, 0, 1]                                         # Kp's plan i is K's plan perm[i]
    for e in range(5):
        for i, j in enumerate(perm):
            assert np.array_equal(Kp.regret(e, i), K.regret(e, j))
            assert np.array_equal(Kp.regret_variance(e, i), K.regret_variance(e, j))        # M2 included
            assert np.array_equal(Kp.counts(e, i), K.counts(e, j))
            for k in range(2):
                assert np.array_equal(Kp.counts(e, 3 + 5 * k + i), K.counts(e, 3 + 5 * k + j))
        for k in range(2):
            assert np.array_equal(Kp.counts(e, 3 + 5 * k + 3), K.counts(e, 3 + 5 * k + 3))
            assert np.array_equal(Kp.counts(e, 3 + 5 * k + 4), K.counts(e, 3 + 5 * k + 4))
    for k in range(2):
        assert np.array_equal(Kp.coverage(k)[0], K.coverage(k)[0][:, perm])


def test_a_twin_plan_is_never_alone(fed):
    Kt, Xba = fed.Ktwin, fed.Xba
    assert max(Xba.counts(e, 0).max() for e in range(5)) > 0 and max(Kt.regret(e, 0).max() for e in range(5)) > 0
    for e in range(5):
        assert not Kt.counts(e, 0).any() and not Kt.counts(e, 1).any()
        assert np.array_equal(Kt.counts(e, 2), Xba.counts(e, 0))                                     # B > A
        assert np.array_equal(Kt.regret(e, 0), Kt.regret(e, 1))
        assert np.array_equal(Kt.regret_variance(e, 0), Kt.regret_variance(e, 1))
        for k in range(2):
            assert not Kt.counts(e, 3 + 5 * k).any() and not Kt.counts(e, 3 + 5 * k + 1).any()
    assert np.array_equal(Kt.coverage(0)[0][:, 0], Kt.coverage(0)[0][:, 1])


def test_doubling_every_amount_and_threshold(fed):
    K, Kd = fed.K, fed.Kdouble
    assert np.array_equal(fed.doubled[1].field(4), 2.0 * fed.B.field(4))
    _same_counts(K, Kd, 5)
    for k in range(2):
        for got, want in zip(Kd.coverage(k), K.coverage(k)):
            assert np.array_equal(got, want)
    for e in range(5):
        for j in range(3):
            assert np.array_equal(Kd.regret(e, j), 2.0 * K.regret(e, j))
            assert np.array_equal(Kd.regret_variance(e, j), 4.0 * K.regret_variance(e, j))
    assert all(max(K.regret_variance(e, j).max() for e in range(5)) > 0 for j in range(3))


def test_weights_merges_and_reset(fed):
    from parasitoids_amd.predictive import PlanRanking
    K, U, lo, hi = fed.K, fed.Kunit, fed.Klo, fed.Khi
    # weight w against w unit adds: the tolerances of the contrast's test
    assert U.total_weight == K.total_weight and U.members == sum(WEIGHTS)
    _same_counts(K, U, 5)
    for e in range(5):
        for j in range(3):
            ma = K.regret(e, j)
            np.testing.assert_allclose(U.regret(e, j), ma, rtol=1e-13, atol=1e-16 * np.abs(ma).max())
            np.testing.assert_allclose(U.regret_variance(e, j), K.regret_variance(e, j), rtol=1e-13,
                                       atol=1e-13 * 1e-3 * np.abs(ma).max() ** 2)
    cells, w = U.coverage(0)
    assert list(w) == [1] * sum(WEIGHTS) and np.array_equal(cells, np.repeat(K.coverage(0)[0], WEIGHTS, axis=0))
    # two handles merged against one over all members
    lo.merge(hi)
    assert lo.total_weight == K.total_weight and lo.members == K.members and hi.members == 3
    _same_counts(K, lo, 5)
    for e in range(5):
        for j in range(3):
            m = K.regret(e, j)
            np.testing.assert_allclose(lo.regret(e, j), m, rtol=1e-12, atol=1e-15 * np.abs(m).max())
            np.testing.assert_allclose(lo.regret_variance(e, j), K.regret_variance(e, j), rtol=1e-12,
                                       atol=1e-15 * np.abs(m).max() ** 2)
    for k in range(2):
        for got, want in zip(lo.coverage(k), K.coverage(k)):
            assert np.array_equal(got, want)                 # the rows in add order, hi's after lo's
    # into an empty handle: a copy, bit for bit; then reset and replay
    with PlanRanking([fed.A, fed.B, fed.C], THR) as E:
        E.merge(K)
        assert E.members == K.members and E.total_weight == K.total_weight
        _same_counts(K, E, 5)
        for e in range(5):
            for j in range(3):
                assert np.array_equal(E.regret(e, j), K.regret(e, j))
                assert np.array_equal(E.regret_variance(e, j), K.regret_variance(e, j))
        for k in range(2):
            for got, want in zip(E.coverage(k), K.coverage(k)):
                assert np.array_equal(got, want)
        E.reset()
        assert E.members == 0 and E.total_weight == 0 and E.coverage(0)[0].shape == (0, 3, 5)
        E.merge(hi)
        _check_exact(E, _replay(fed.fields, WEIGHTS, THR, members=[2, 3, 4]), 5)
        for e in range(5):
            for j in range(3):
                assert np.array_equal(E.regret_variance(e, j) * 4.0, hi.regret_variance(e, j) * 4.0)
        with pytest.raises(ValueError, match='different outputs'):
            E.merge(types.SimpleNamespace(live=[0], nout=1, labels=[0], nplan=3))
        with pytest.raises(ValueError, match='numbers of plans'):
            E.merge(fed.K2)


def test_the_accumulators_beside_a_ranking_are_untouched(fed):
    """plan A's summary, histogram and arrival maps filled alone, from fresh models (an auto-mode model routes
    days by what it has seen before), against those filled beside the rankings"""
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


def test_a_tuple_of_three_projections():
    from parasitoids_amd.predictive import PlanRanking, Projection, ReleaseSites, exposure_weights
    pm = _pop_model(R)
    zero = np.zeros((1, 6))
    Wa = np.concatenate([exposure_weights(DAYS, [0, 2]), zero, exposure_weights(DAYS, [5])])
    Wb = np.concatenate([exposure_weights(DAYS, [1, 3]), zero, exposure_weights(DAYS, [4])])
    Wc = np.concatenate([exposure_weights(DAYS, [0, 4]), zero, exposure_weights(DAYS, [3])])
    thr = [50.0, 500.0]
    fields = []
    with Projection(pm, Wa, DAYS) as PA, Projection(pm, Wb, DAYS) as PB, Projection(pm, Wc, DAYS) as PC, \
            PlanRanking((PA, PB, PC), thr) as K, ReleaseSites(pm, [(0, 0, 1.0)], [0, 1, 2, 3]) as RS:
        assert K.live == [0, 1, 3] and K.nout == 4 and K.labels == [0, 1, 2, 3] and K.names == ['plan0', 'plan1', 'plan2']
        with pytest.raises(ValueError, match='ReleaseSites only or Projection only'):
            PlanRanking([PA, PB, RS])
        with pytest.raises(ValueError, match='listed twice'):
            PlanRanking([PA, PB, PA])
        with pytest.raises(ValueError, match='one per plan'):
            PlanRanking([PA, PB, PC], thr, ['x', 'y'])
        with Projection(pm, Wa[:2], DAYS) as short, pytest.raises(ValueError, match='differ in nout'):
            PlanRanking([PA, PB, short])
        with ReleaseSites(pm, [(0, 0, 0.5)], [0, 1, 2, 5]) as other, ReleaseSites(pm, [(0, 0, 0.7)], [0, 1, 2, 3]) as same, \
                pytest.raises(ValueError, match='differ in days'):
            PlanRanking([RS, same, other])                   # as many outputs, other days: not paired by index
        for mem, w in zip(MEMBERS[:3], WEIGHTS[:3]):
            _evaluate(pm, mem)
            for P in (PA, PB, PC):
                P.apply()
            K.add(w)
            fields.append([[P.field(e) for P in (PA, PB, PC)] for e in range(4)])
        ref = _replay(fields, WEIGHTS[:3], thr)
        # up to day 0 against up to day 1: B ahead everywhere it reaches, A and C tied behind it; up to day 5: A ahead
        assert ref[0]['best'][1].max() == 5 and not ref[0]['best'][0].any() and not ref[0]['best'][2].any()
        assert ref[3]['best'][0].max() == 5 and ref[0]['sole'][1, 1].max() > 0
        assert np.array_equal(ref[0]['mean'][0], ref[0]['mean'][2]) and ref[0]['mean'][0].max() > 0
        assert not fields[0][2][0].any() and not ref[2]['mean'].any() and ref[2]['cells'] == [[[0, 0]] * 3] * 3
        _check_exact(K, ref, 4)
        _check_variance(K, fields, WEIGHTS[:3], 4)
        assert (K.leader(2) == -1).all() and (K.prob_undecided(2) == 1.0).all()
    pm.close()


def test_posterior_predictive_with_ranked_plans(tmp_path, monkeypatch):
    from parasitoids_amd import mcmc
    from parasitoids_amd import predictive as PR
    trace, names = _chain([2, 1, 3, 1, 2])
    chains = [(trace[:5], names), (trace[5:], names)]
    plan_b = [(0, 0, 1.5, 0), (-5, 3, 0.5, 2), (7, -4, 0.25, 3)]
    plan_c = [(0, 0, 1.25, 0), (4, 9, 0.5, 1)]
    plan_d = [(0, 0, 0.6, 0), (0, 13, 0.4, 0), (-9, 6, 0.5, 2)]         # A's first two sites: positive ties with A

    def as_arg(cells):
        return [s[:3] + ((s[3],) if s[3] else ()) for s in _metres(cells, R)]
    arg = dict(sites=as_arg(STAGGERED), days=OUT)
    cmp_arg = dict(sites=as_arg(plan_b))
    rk_arg = dict(plans=[dict(sites=as_arg(plan_c)), dict(sites=as_arg(plan_d))], names=['now', 'near', 'north'],
                  levels=(0.5,))
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
                assert k.get('ndays') == OUT[-1] - _key[1] + 1
                return _inner(*a, **k)
            m.evaluate = evaluate
        return made
    monkeypatch.setattr(PR, 'lagged_models', counting)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        pa, pb, pd = (_pop_model(R, mode='exact') for _ in range(3))
        res = PR.posterior_predictive(pa, chains, sites=arg, compare=cmp_arg, ranking=rk_arg, **kw)
        # sites= has the lags 0, 2; compare= 0, 2, 3; the ranked plans 0, 1 and 0, 2: one model per lag, once per member
        assert made_for == [(pa, [1, 2, 3])] and calls == {(id(pa), lag): 6 for lag in (1, 2, 3)}
        bare = PR.posterior_predictive(pb, chains[:1], sites=arg, ranking=rk_arg['plans'], **kw)     # the shorthand
        assert made_for[1] == (pb, [1, 2]) and all(calls[(id(pb), lag)] == 3 for lag in (1, 2))
        plain = PR.posterior_predictive(pd, chains, sites=arg, compare=cmp_arg, **kw)
    monkeypatch.setattr(PR, 'lagged_models', real)
    K = res.ranking
    assert plain.ranking is None and plain.ranking_plans is None and res.failed == 0 and len(res.runs) == 6
    assert K.total_weight == 9 and K.members == 6 and K.labels == OUT and K.thresholds == THR and K.nplan == 3
    assert K.names == ['now', 'near', 'north'] and res.ranking_levels == [0.5]
    assert bare.ranking.names == ['plan0', 'plan1', 'plan2'] and bare.ranking.members == 3 and bare.contrast is None
    assert [p['lags'] for p in res.ranking_plans] == [[0, 2], [0, 1], [0, 2]]
    assert all(p['days'] == OUT for p in res.ranking_plans)
    assert [(s['drow'], s['dcol'], s['amount'], s['lag']) for s in res.ranking_plans[1]['sites']] == plan_c
    # plan A's own maps and the contrast do not know about the ranking
    for e in range(5):
        assert np.array_equal(res.sites.summary.mean(e), plain.sites.summary.mean(e))
        assert np.array_equal(res.sites.summary.variance(e), plain.sites.summary.variance(e))
        assert np.array_equal(res.sites.arrival.counts(1, OUT[e]), plain.sites.arrival.counts(1, OUT[e]))
        assert np.array_equal(res.contrast.mean(e), plain.contrast.mean(e))
        assert np.array_equal(res.contrast.variance(e), plain.contrast.variance(e))
    # by hand: one ranking per chain, merged in chain order
    cols = [names.index(m[0]) for m in mcmc.MODEL_BLOCK]
    pm = _pop_model(R, mode='exact')
    late = real(pm, [1, 2, 3])
    fields, wts = [], []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        with PR.ReleaseSites(pm, arg['sites'], OUT, late) as A, PR.ReleaseSites(pm, as_arg(plan_c), OUT, late) as Cp, \
                PR.ReleaseSites(pm, as_arg(plan_d), OUT, late) as D, PR.PlanRanking([A, Cp, D], THR) as M0, \
                PR.PlanRanking([A, Cp, D], THR) as M1:
            for ci, first, weight in res.runs:
                args = mcmc.model_args(chains[ci][0][first, cols])
                pm.evaluate(*args, want_stats=False)
                for lag, m in sorted(late.items()):
                    m.evaluate(*args, ndays=OUT[-1] - lag + 1, want_stats=False)
                for plan in (A, Cp, D):
                    plan.apply()
                (M0, M1)[ci].add(weight)
                fields.append([[plan.field(e) for plan in (A, Cp, D)] for e in range(5)])
                wts.append(weight)
            M0.merge(M1)
            ref = _replay(fields, wts, THR)
            assert all(max(st['best'][j].max() for st in ref) > 0 for j in range(3))
            assert all(max(st['sole'][k].max() for st in ref) > 0 for k in range(2))
            top = np.array(fields).max(axis=2)
            assert (((np.array(fields) == top[:, :, None]).sum(axis=2) > 1) & (top > 0)).any()      # a positive tie
            for got in (K, M0):
                for e in range(5):
                    planes = rank_ref.planes(ref[e])
                    for which in range(K.nplanes):
                        assert np.array_equal(got.counts(e, which).astype(np.int64), planes[which]), (e, which)
                    for j in range(3):
                        m = M0.regret(e, j)
                        if got is not M0:
                            # the same adds per chain and the same merge in chain order, in exact mode, from fresh
                            # models per path: the driver equals the manual loop bit for bit
                            assert np.array_equal(got.regret(e, j), m), (e, j)
                            assert np.array_equal(got.regret_variance(e, j), M0.regret_variance(e, j)), (e, j)
                        # the unmerged replay over all six members: the merge re-associates
                        np.testing.assert_allclose(got.regret(e, j), ref[e]['mean'][j], rtol=1e-12,
                                                   atol=1e-15 * np.abs(m).max())
                for k in range(2):
                    cells, w = got.coverage(k)
                    assert list(w) == wts
                    assert np.array_equal(cells, np.stack([rank_ref.rows(st)[:, :, k] for st in ref], axis=2))
            first = _replay(fields, wts, THR, members=[0, 1, 2])      # the chain of one: the first three members
            for e in range(5):
                for j in range(3):
                    assert np.array_equal(bare.ranking.counts(e, j).astype(np.int64), first[e]['best'][j])
    # the result files
    npz, js = res.save(str(tmp_path / 'a' / 'pp'))
    plain.save(str(tmp_path / 'p' / 'pp'))
    assert not os.path.exists(str(tmp_path / 'p' / 'pp_ranking.npz'))
    assert sorted(os.listdir(str(tmp_path / 'a'))) == sorted(os.listdir(str(tmp_path / 'p')) + ['pp_ranking.npz'])
    for name in ('pp.npz', 'pp_sites.npz', 'pp_contrast.npz'):     # the other files do not know about the ranking
        with np.load(str(tmp_path / 'a' / name)) as fx, np.load(str(tmp_path / 'p' / name)) as fp:
            assert set(fx.files) == set(fp.files)
            for key in fp.files:
                assert np.array_equal(fx[key], fp[key]), key
    with np.load(str(tmp_path / 'a' / 'pp_ranking.npz')) as fz:
        assert [int(x) for x in fz['days']] == OUT
        want = {'days', 'ranking_weights', 'coverage0', 'coverage1'}
        for e, lab in enumerate(OUT):
            maps = []
            for j in range(3):
                maps += [('_pbest%d' % j, K.prob_best(e, j)), ('_regret%d' % j, K.regret(e, j)),
                         ('_regret_sd%d' % j, K.regret_sd(e, j)), ('_psole0_%d' % j, K.sole(e, 0, j)),
                         ('_psole1_%d' % j, K.sole(e, 1, j))]
            for k in range(2):
                maps += [('_pany%d' % k, K.any(e, k)), ('_pall%d' % k, K.all(e, k))]
            for suffix, m in maps:
                assert np.array_equal(_csr(fz, '%d%s' % (lab, suffix), N), np.where(m >= 1e-8, m, 0.0)), (lab, suffix)
                want |= {'%d%s_%s' % (lab, suffix, t) for t in ('data', 'ind', 'indptr')}
            assert fz['%d_leader' % lab].dtype == np.int8 and np.array_equal(fz['%d_leader' % lab], K.leader(e))
            want.add('%d_leader' % lab)
        assert set(fz.files) == want
        assert fz['coverage1'].shape == (6, 3, 5) and np.array_equal(fz['coverage1'], K.coverage(1)[0])
        assert list(fz['ranking_weights']) == wts
    mr = json.load(open(js))['predictive']['ranking']
    assert [p['lags'] for p in mr['plans']] == [[0, 2], [0, 1], [0, 2]] and mr['names'] == ['now', 'near', 'north']
    assert mr['thresholds'] == THR and mr['labels'] == OUT and mr['members'] == 6 and mr['total_weight'] == 9
    assert mr['cell_area'] == K.cell_area and mr['levels'] == [0.5]
    assert mr['coverage_ranking'] == [K.coverage_ranking(k, (0.5,)) for k in range(2)]
    plain_meta = json.load(open(str(tmp_path / 'p' / 'pp.json')))['predictive']
    assert 'ranking' not in plain_meta
    assert plain_meta['contrast'] == json.load(open(js))['predictive']['contrast']
    # a model of the union that fails for one member leaves that member out of every accumulator: lag 1 is the
    # ranked plan C's alone, so plan A's maps and the day-based ones skip the member too
    seen = []

    def failing(pop_model, lags, wind_data=None):
        made = real(pop_model, lags, wind_data)
        inner = made[1].evaluate

        def evaluate(*a, **k):
            seen.append(1)
            if len(seen) == 2:
                raise ValueError('no kernel for this member')
            return inner(*a, **k)
        made[1].evaluate = evaluate
        return made
    monkeypatch.setattr(PR, 'lagged_models', failing)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        pe = _pop_model(R, mode='exact')
        part = PR.posterior_predictive(pe, chains[:1], sites=arg, ranking=rk_arg, **kw)
    monkeypatch.setattr(PR, 'lagged_models', real)
    assert part.failed == 1 and part.evaluations == 3 and [r[1:] for r in part.runs] == [(0, 2), (3, 2)]
    for acc in (part.summary, part.arrival, part.sites.summary, part.sites.arrival, part.ranking):
        assert acc.members == 2 and acc.total_weight == 4
    assert list(part.ranking.weights) == [2, 2]
    _check_exact(part.ranking, _replay([fields[0], fields[2]], [2, 2], THR), 5)
    for r in (res, bare, plain, part):
        for acc in (r.summary, r.arrival, r.sites, r.contrast, r.ranking):
            if acc is not None:
                acc.close()
    for p in (pm, pa, pb, pd, pe) + tuple(late.values()):
        p.close()


def _handles(*plans):
    return (C.c_void_p * len(plans))(*[None if p is None else p._h.value for p in plans])


def test_refusals_at_the_c_abi_and_the_handle_stays_usable():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import PlanRanking, Projection, ReleaseSites, exposure_weights, lagged_models
    lib = L.load()
    dev = L.default_device()
    h = L._VP()

    def create(thr, nplan=3, N=129, nslot=3, device=dev):
        t = L.f64(thr if len(thr) else [0.0])
        return lib.ps_rank_create(device, N, nplan, nslot, len(thr), L.p_f64(t), C.byref(h))
    assert create([1, 2, 3, 4, 5]) == L.PS_ERR_BAD_ARG and not h
    for bad in ([0.0], [-1.0], [np.nan], [np.inf], [1.0, 1.0], [2.0, 1.0]):
        assert create(bad) == L.PS_ERR_BAD_ARG and not h
    assert b'threshold' in lib.ps_last_error()
    for nplan in (-1, 0, 1, 9):
        assert create([1.0], nplan=nplan) == L.PS_ERR_BAD_ARG and not h
        assert b'plans' in lib.ps_last_error()
    assert create([1.0], nslot=0) == L.PS_ERR_BAD_ARG and not h
    assert create([1.0], device=99) == L.PS_ERR_NO_DEVICE and not h
    assert create([1.0, 2.0, 3.0, 4.0], nplan=8, N=60001, nslot=32) == L.PS_ERR_OOM and not h      # 37 TB
    assert b'GB free' in lib.ps_last_error()
    for nplan in (2, 8):
        assert create([], nplan=nplan) == L.PS_OK and h
        lib.ps_rank_destroy(h)
    pm, big = _pop_model(R), _pop_model(128)
    late = lagged_models(pm, [2])
    cells = [(0, 0, 1.0, 0), (3, 5, 0.5, 0)]
    out = np.empty((N, N))
    cnt = np.empty((N, N), dtype=np.uint32)
    u32 = C.POINTER(C.c_uint32)
    with ReleaseSites(pm, _metres(cells, R), [0, 2, 5]) as A, ReleaseSites(pm, _metres(cells[:1], R), [0, 2, 5]) as B, \
            ReleaseSites(pm, _metres(cells[1:], R), [0, 2, 5]) as Cp, \
            ReleaseSites(big, _metres(cells, 128), [0, 2, 5]) as B128, ReleaseSites(pm, _metres(cells, R), [0, 2]) as B2, \
            ReleaseSites(pm, _metres(STAGGERED, R), [0, 2, 5], late) as Bst, \
            Projection(pm, exposure_weights(DAYS, [0, 2, 5]), DAYS) as PA, \
            Projection(pm, exposure_weights(DAYS, [1, 2, 5]), DAYS) as PB, PlanRanking([A, B, Cp], THR) as K:
        K.profile(True)
        # before the first add, and before the plans hold anything
        assert lib.ps_rank_fetch(K._h, 0, 0, 0, L.p_f64(out)) == L.PS_ERR_STATE
        assert lib.ps_rank_fetch_counts(K._h, 0, 0, cnt.ctypes.data_as(u32)) == L.PS_ERR_STATE
        assert lib.ps_rank_add_sites(K._h, _handles(A, B, Cp), 3, 1) == L.PS_ERR_STATE
        for m in (pm, big):
            _evaluate(m, MEMBERS[0])
        _evaluate(late[2], MEMBERS[0], ndays=4)
        for plan in (A, B, B128, B2):
            plan.apply()
        assert lib.ps_rank_add_sites(K._h, _handles(A, B, Cp), 3, 1) == L.PS_ERR_STATE       # C not applied yet
        Cp.apply()
        L.check(lib.ps_sites_apply(Bst._h, *Bst._calls()[0]))
        assert lib.ps_rank_add_sites(K._h, _handles(A, B, Bst), 3, 1) == L.PS_ERR_STATE      # mid-pass over its groups
        assert b'group 1 of 2' in lib.ps_last_error()
        assert lib.ps_rank_add_sites(K._h, _handles(Bst, A, B), 3, 1) == L.PS_ERR_STATE
        for plans, n, w, msg in (((A, B, A), 3, 1, b'0 and 2 are the same handle'), ((A, A, B), 3, 1, b'0 and 1 are the same'),
                                 ((A, B, B128), 3, 1, b'domain 257'), ((B128, A, B), 3, 1, b'domain 257'),
                                 ((A, B2, B), 3, 1, b'has 2 outputs'), ((A, B, Cp), 3, 0, b'weight must be >= 1'),
                                 ((A, None, B), 3, 1, b'1 is null'), ((None, A, B), 3, 1, b'0 is null'),
                                 ((A, B), 2, 1, b'2 plans given, the handle ranks 3'),
                                 ((A, B, Cp, B2), 4, 1, b'4 plans given'), ((A, B, Cp), 1, 1, b'1 plans given'),
                                 ((A, B, Cp), 9, 1, b'9 plans given'), ((A, B, Cp), 0, 1, b'0 plans given')):
            assert lib.ps_rank_add_sites(K._h, _handles(*plans), n, w) == L.PS_ERR_BAD_ARG, msg
            assert msg in lib.ps_last_error(), (msg, lib.ps_last_error())
        assert lib.ps_rank_add_sites(None, _handles(A, B, Cp), 3, 1) == L.PS_ERR_BAD_ARG
        assert lib.ps_rank_add_sites(K._h, None, 3, 1) == L.PS_ERR_BAD_ARG
        assert lib.ps_rank_add_project(K._h, _handles(PA, PB, PA), 3, 1) == L.PS_ERR_BAD_ARG      # a projection twice
        assert K.members == 0 and K.total_weight == 0 and K.profile()[1] == 0             # nothing was enqueued
        K.add(2)
        assert lib.ps_rank_add_sites(K._h, _handles(A, B, Cp), 3, 0xfffffffe) == L.PS_ERR_BAD_ARG  # W past 2^32 - 1
        assert b'overflow' in lib.ps_last_error()
        for slot, plan, what in ((-1, 0, 0), (3, 0, 0), (0, -1, 0), (0, 3, 0), (0, 0, -1), (0, 0, 3)):
            assert lib.ps_rank_fetch(K._h, slot, plan, what, L.p_f64(out)) == L.PS_ERR_BAD_ARG
        for slot, which in ((3, 0), (-1, 0), (0, -1), (0, 13)):
            assert lib.ps_rank_fetch_counts(K._h, slot, which, cnt.ctypes.data_as(u32)) == L.PS_ERR_BAD_ARG
        assert lib.ps_rank_fetch_coverage(K._h, 0, 2, None, None) == L.PS_ERR_BAD_ARG
        assert lib.ps_rank_fetch_coverage(K._h, -1, 1, None, None) == L.PS_ERR_BAD_ARG
        with PlanRanking([A, B, Cp], [1.0]) as other, PlanRanking([A, B], THR) as two:
            assert lib.ps_rank_merge(K._h, other._h) == L.PS_ERR_BAD_ARG               # other thresholds
            assert lib.ps_rank_merge(K._h, two._h) == L.PS_ERR_BAD_ARG                 # another number of plans
        assert lib.ps_rank_merge(K._h, K._h) == L.PS_ERR_BAD_ARG
        assert K.members == 1 and K.total_weight == 2 and K.profile()[1] == 1
        # the handle still works: one member of weight 2
        fields = [[[p.field(e) for p in (A, B, Cp)] for e in range(3)]]
        _check_exact(K, _replay(fields, [2], THR), 3)
        assert not K.regret_variance(1, 1).any() and K.counts(2, 0).max() == 2 and not K.counts(2, 1).any()
    for m in (pm, big, late[2]):
        m.close()


def test_the_grid_stride_path():
    """at R = 64 every launch is a single pass; the cell counts carried in registers over the grid stride only
    show once the pairs of cells exceed the launch cap of 4096 x 256, from R = 724 on: R = 768, 2 days, 2 members,
    three single-group plans, plan B with a site on the south-east corner so that the tail cell counts too"""
    from parasitoids_amd.predictive import PlanRanking, ReleaseSites
    big = 768
    n = 2 * big + 1
    assert (n * n) // 2 > 4096 * 256 and (n * n) % 2 == 1
    pm = _pop_model(big, ndays=2)
    plan_a = [(0, 0, 1.0, 0), (700, -25, 0.5, 0)]                    # the second site beyond the grid's first pass
    plan_b = [(0, 0, 0.7, 0), (-30, 60, 0.8, 0), (big, big, 0.5, 0)]
    plan_c = [(0, 0, 0.9, 0), (700, -25, 0.5, 0), (690, 40, 0.6, 0)]  # ties with A beyond the first pass
    thr = [1.0, 100.0]
    fields = []
    with ReleaseSites(pm, _metres(plan_a, big), [0, 1]) as A, ReleaseSites(pm, _metres(plan_b, big), [0, 1]) as B, \
            ReleaseSites(pm, _metres(plan_c, big), [0, 1]) as Cp, PlanRanking([A, B, Cp], thr) as K:
        assert [(s['drow'], s['dcol']) for s in B.sites] == [c[:2] for c in plan_b]
        for mem, w in zip(MEMBERS[:2], WEIGHTS[:2]):
            _evaluate(pm, mem)
            for plan in (A, B, Cp):
                plan.apply()
            K.add(w)
            fields.append([[plan.field(e) for plan in (A, B, Cp)] for e in range(2)])
        ref = _replay(fields, WEIGHTS[:2], thr)
        assert fields[0][0][1][n - 1, n - 1] >= thr[1] and ref[0]['best'][1][n - 1, n - 1] == 4
        assert ref[0]['sole'][1, 1][n - 1, n - 1] == 4
        # cells beyond the first pass of the grid (flat index >= 2 x 4096 x 256) in the rows and in the planes
        first_pass = 2 * 4096 * 256
        for j in (0, 2):
            assert (fields[0][1][j].ravel()[first_pass:] >= thr[0]).sum() > 0
        assert ref[1]['best'][2].ravel()[first_pass:].max() > 0 and ref[1]['any'][0].ravel()[first_pass:].max() > 0
        _check_exact(K, ref, 2)
    pm.close()
