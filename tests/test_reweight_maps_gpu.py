"""GPU tests of the reweighted quantile and arrival maps (ps_whist_* / ps_warr_*, predictive.ReweightedHistogram /
ReweightedArrival): every plane bit for bit against the numpy loops of whist_ref / warr_ref on
`PopModel.population(d)`, the readings against the references evaluated on those planes, the tie of an all-zero
scenario to SpreadHistogram / ArrivalMaps, the exceedance against ReweightedSummary's, add and merge order,
projections and release plans as sources, the reached-area curve, the refusals, and posterior_predictive with
reweight's maps option.  Kalbar wind, R = 128, 6 days (N = 257: N * N is odd, the tail cell is on its own), the
members and weights of test_arrival_gpu.py and the log-weights of test_reweight_gpu.py."""
import json
import math
import os
import types
import warnings

import numpy as np
import pytest

import arrival_ref as AR
import reweight_ref as RR
import warr_ref as WA
import whist_ref as WH
from helpers import HP, DLP, NPER
from test_arrival_gpu import MEMBERS, WEIGHTS, THR, _pop_model, _evaluate, _fields
from test_reweight_gpu import LAM, NAMES, _chain, _check_close, _csr

pytestmark = pytest.mark.gpu

INF = math.inf
LEVELS = (0.05, 0.3, 0.5, 0.95, 1.0)
EDGES2 = [1.0, 10.0]                                          # the smallest table: the summary's two thresholds
EDGES9 = [1e-6, 1e-4, 1e-2, 1e-1, 1.0, 10.0, 100.0, 1e3, 1e4]    # edges 4 and 5 are the summary's thresholds
LAM4 = dict(LAM, shifted=[l + 256.0 for l in LAM['swing']])
NAMES4 = NAMES + ['shifted']


def _lams(names, m):
    return [LAM4[n][m] for n in names]


def _host(R, st, names):
    """ref, W, members and skipped of every scenario against a reference state, bit for bit"""
    for j, n in enumerate(names):
        sc = st[j]
        assert R.ref[j] == sc['ref'] and R.total_weight(n) == sc['W'], n
        assert (R.members(n), R.skipped(n)) == (sc['members'], sc['skipped']), n
        assert R.log_total_weight(n) == RR.log_total_weight(sc), n


def _check_hist(H, st, names, keys, levels=LEVELS, exceed=None):
    """every plane of H against the loop, and b*, bracket, exceedance and point value against the reference
    evaluated on those planes (the point value by the rule of test_spread_histogram_gpu.py: rtol 1e-12)"""
    edges = H.edges
    _host(H, st, names)
    for j, n in enumerate(names):
        sc = st[j]
        for i, d in enumerate(keys):
            for b in range(1, edges.size + 1):
                assert np.array_equal(H.plane(n, d, b), sc['H'][b, i]), (n, d, b)
            if sc['W'] == 0.0:
                continue
            planes = sc['H'][:, i]
            for p in levels:
                bs, val, lo, hi, _near = WH.quantile_from_planes(planes, sc['W'], edges, p)
                gv, glo, ghi = H.quantile(n, d, p)
                assert np.array_equal(H.quantile_bin(n, d, p), bs), (n, d, p)
                assert np.array_equal(glo, lo) and np.array_equal(ghi, hi), (n, d, p)
                np.testing.assert_allclose(gv, val, rtol=1e-12, atol=0)
                # inside its bracket, up to the rounding of e (e' / e)^f at f = 0 or 1: a division, a pow and a
                # product, 1e-15 relative between them
                assert np.all((glo * (1 - 1e-15) <= gv) & ((gv <= ghi * (1 + 1e-15)) | (ghi == np.inf)))
            for k in (range(edges.size) if exceed is None else exceed):
                assert np.array_equal(H.exceed(n, d, k), WH.exceedance_from_planes(planes, sc['W'], k)), (n, d, k)


def _check_arr(A, st, names, levels=LEVELS):
    """every plane of A against the loop, prob_by and the quantile days against the reference on those planes"""
    _host(A, st, names)
    days = A.days
    for j, n in enumerate(names):
        sc = st[j]
        for k in range(len(A.thresholds)):
            for s, d in enumerate(days):
                assert np.array_equal(A.plane(n, k, d), sc['A'][k, s]), (n, k, d)
            if sc['W'] == 0.0:
                continue
            P = WA.probability(sc['A'][k], sc['W'])
            for s, d in enumerate(days):
                assert np.array_equal(A.prob_by(n, k, d), P[s]), (n, k, d)
            for p in levels:
                q = WA.quantile_slots(sc['A'][k], sc['W'], p)
                want = np.where(q < 0, -1, np.asarray(days)[q.clip(0)])
                got = A.quantile(n, k, p)
                assert got.dtype == np.int32 and np.array_equal(got, want), (n, k, p)


def test_three_scenarios_match_the_numpy_loop_and_tie_to_the_integer_accumulators():
    from parasitoids_amd.predictive import (ArrivalMaps, ReweightedArrival, ReweightedHistogram, ReweightedSummary,
                                            SpreadHistogram, weighted_lower_quantile)
    pm = _pop_model()
    days = list(range(6))
    N, pitch = 257, 66112
    sh = WH.new_state((6, N, N), EDGES9, 3)
    sa = WA.new_state((6, N, N), THR, 3)
    sh1 = WH.new_state((6, N, N), EDGES2, 1)
    sa1 = WA.new_state((6, N, N), THR[:1], 1)
    fields = []
    with ReweightedHistogram(pm, NAMES, days, edges=EDGES9) as H, ReweightedArrival(pm, NAMES, THR, days) as A, \
            ReweightedHistogram(pm, ['swing'], None, edges=EDGES2) as H1, ReweightedArrival(pm, ['swing'], THR[:1]) as A1, \
            ReweightedSummary(pm, NAMES, days, THR) as S, SpreadHistogram(pm, days, edges=EDGES9) as G, \
            ArrivalMaps(pm, THR, days) as B:
        assert H.N == N and H.scenarios == NAMES and H.nbytes == 3 * 6 * 9 * pitch * 8 + 6 * pitch * 4
        assert A.nbytes == 3 * 2 * 6 * pitch * 8 and H1.days == days and A1.days == days
        assert H.log_total_weight('late') == -INF and A.ref == [-INF] * 3
        for m, (mem, w) in enumerate(zip(MEMBERS, WEIGHTS)):
            _evaluate(pm, mem)
            lam = _lams(NAMES, m)
            for acc in (H, A, S):
                acc.add(lam, w)
            H1.add([LAM['swing'][m]], w)
            A1.add({'swing': LAM['swing'][m]}, w)
            G.add(w)
            B.add(w)
            f = _fields(pm, days)
            fields.append(f)
            WH.add(sh, f, lam, w)
            WA.add(sa, f, lam, w)
            WH.add(sh1, f, [LAM['swing'][m]], w)
            WA.add(sa1, f, [LAM['swing'][m]], w)
        # 1, 2: the planes and the host side bit for bit, the readings from those planes
        _check_hist(H, sh, NAMES, days)
        _check_arr(A, sa, NAMES)
        _check_hist(H1, sh1, ['swing'], days, levels=(0.5, 1.0))
        _check_arr(A1, sa1, ['swing'], levels=(0.5,))
        assert H.ref == [0.0, 2.25, 3.0] == A.ref == S.ref
        for n in NAMES:                      # against the ReweightedSummary fed alongside
            for R in (H, A):
                assert (R.total_weight(n), R.members(n), R.skipped(n)) == (S.total_weight(n), S.members(n), S.skipped(n))
                assert R.log_total_weight(n) == S.log_total_weight(n)
        assert [H.members(n) for n in NAMES] == [5, 4, 4] and [A.skipped(n) for n in NAMES] == [0, 1, 1]
        assert H.plane('swing', 5, 5).max() > 0 and A.plane('late', 1, 4).max() > 0
        assert not np.array_equal(H.quantile('swing', 5, 0.5)[0], H.quantile('flat', 5, 0.5)[0])
        assert not np.array_equal(A.prob_by('swing', 0, 3), A.prob_by('flat', 0, 3))
        # 3: the all-zero scenario is the integer accumulator fed alongside, bit for bit, point value included
        for d in days:
            cnt = G.counts(d)
            for b in range(1, 10):
                assert np.array_equal(H.plane('flat', d, b), cnt[b].astype(np.float64)), (d, b)
            for p in LEVELS:
                v, lo, hi = H.quantile('flat', d, p)
                glo, ghi = G.quantile_bounds(d, p)
                assert np.array_equal(v, G.quantile(d, p)) and np.array_equal(lo, glo) and np.array_equal(hi, ghi), (d, p)
            for k, e in enumerate(EDGES9):
                assert np.array_equal(H.exceed('flat', d, k), G.exceedance(d, e)), (d, k)
            for k in range(2):
                assert np.array_equal(A.plane('flat', k, d), B.counts(k, d).astype(np.float64)), (k, d)
                assert np.array_equal(A.prob_by('flat', k, d), B.prob_by(k, d)), (k, d)
        for k in range(2):
            for p in LEVELS:
                assert np.array_equal(A.quantile('flat', k, p), B.quantile(k, p)), (k, p)
        # 4: the exceedance at an edge that is a summary threshold.  Both sum the same non-negative terms -- the
        # summary one sum per threshold in add order, the histogram one sum per bin and then the bins from the top --
        # so they agree within the rounding of those sums, not bit for bit: each of the at most M adds of a plane,
        # the B + 1 adds of the tail and the two divisions is within 2^-53, 2 (M + B + 2) 2^-53 = 3.6e-15 < 1e-14
        # for M = 5 members and B + 1 = 9 edges.
        for n in NAMES:
            for d in days:
                for k, e in ((0, 4), (1, 5)):
                    np.testing.assert_allclose(H.exceed(n, d, e), S.exceedance(n, d, k), rtol=1e-14, atol=0)
        # 7: the reached-area curve under 'swing', from the rows of the ArrivalMaps fed alongside
        rows = AR.reached_rows(fields, THR)
        assert A.member_log_weights('swing') == [(l, float(w)) for l, w in zip(LAM['swing'], WEIGHTS)]
        wts = np.array([0.0 if l == -INF else w * math.exp(l - 2.25) for l, w in zip(LAM['swing'], WEIGHTS)])
        assert wts[4] == 0.0 and np.array_equal(A.member_weights('swing'), wts)
        for k in range(2):
            curve = A.reached_area('swing', k, B, (0.05, 0.5, 0.95))
            plain = B.reached_area(k, (0.05, 0.5, 0.95))
            for s, d in enumerate(days):
                want = [float(weighted_lower_quantile(rows[:, k, s], wts, p)) * A.cell_area for p in (0.05, 0.5, 0.95)]
                assert curve[s]['day'] == d and curve[s]['quantiles'] == want, (k, d)
            assert [c['quantiles'] for c in curve] != [c['quantiles'] for c in plain]
            # at level 1 the largest reached area among the members that carry weight, by no code of the package
            top = A.reached_area('swing', k, B, (1.0,))
            assert [c['quantiles'][0] for c in top] == [float(rows[wts > 0, k, s].max()) * A.cell_area for s in range(6)]
            assert [c['quantiles'] for c in A.reached_area('flat', k, B)] == [c['quantiles'] for c in plain]
        with ArrivalMaps(pm, THR, days) as short:
            short.add(1)
            with pytest.raises(ValueError, match='5 members'):
                A.reached_area('swing', 0, short)
        # a dict of log-weights by name, and reset
        A.reset()
        H.reset()
        assert A.ref == [-INF] * 3 and H.members('flat') == 0 and A.member_log_weights('flat') == []
        H.add({'late': 0.0, 'flat': -1.0, 'swing': -INF}, 2)
        assert (H.members('swing'), H.skipped('swing'), H.ref) == (0, 1, [-1.0, -INF, 0.0])
        assert np.array_equal(H.plane('late', 3, 5), H.plane('flat', 3, 5)) and H.total_weight('flat') == 2.0
    pm.close()


def test_four_scenarios_on_the_default_edges_and_a_probability_model():
    """J = 4 on the default 225 edges over two slots, K = 1; the probability model's records carry a delta"""
    from parasitoids_amd.predictive import DEFAULT_BINS, ReweightedArrival, ReweightedHistogram, bin_edges
    pm = _pop_model(prob_model=True)
    days = [2, 5]
    edges = bin_edges(DEFAULT_BINS)
    thr = [1.0 / 130000]
    sh = WH.new_state((2, 257, 257), edges, 4)
    sa = WA.new_state((2, 257, 257), thr, 4)
    with ReweightedHistogram(pm, NAMES4, days) as H, ReweightedArrival(pm, NAMES4, thr, days) as A:
        assert H.edges.size == 225 and H.nbytes == 4 * 2 * 225 * 66112 * 8 + 2 * 66112 * 4
        for m, (mem, w) in enumerate(zip(MEMBERS, WEIGHTS)):
            _evaluate(pm, mem)
            lam = _lams(NAMES4, m)
            H.add(lam, w)
            A.add(lam, w)
            f = _fields(pm, days)
            WH.add(sh, f, lam, w)
            WA.add(sa, f, lam, w)
        assert any(pm.stats[d].delta != 0.0 for d in range(5))
        _check_hist(H, sh, NAMES4, days, levels=(0.05, 0.5, 0.95), exceed=(0, 100, 128, 224))
        _check_arr(A, sa, NAMES4, levels=(0.5, 0.95))
        assert H.ref == [0.0, 2.25, 3.0, 258.25] and H.skipped('shifted') == 1
        # a common shift of the log-weights by a power of two changes no plane: every r and omega is the same
        assert H.total_weight('shifted') == H.total_weight('swing')
        for i, d in enumerate(days):
            held = np.flatnonzero(sh[1]['H'][:, i].reshape(226, -1).any(1))
            assert held.size > 3
            for b in held[[0, held.size // 2, -1]]:
                assert np.array_equal(H.plane('shifted', d, int(b)), H.plane('swing', d, int(b))), (d, b)
        assert H.exceed('swing', 5, 0).max() > 0
    pm.close()


def test_the_slot_walk_over_eighteen_days():
    from parasitoids_amd.predictive import ArrivalMaps, ReweightedArrival, ReweightedHistogram
    names = ['swing', 'late', 'flat']
    pm = _pop_model(R=64, ndays=18)
    days = list(range(18))
    sa = WA.new_state((18, 129, 129), THR, 3)
    sh = WH.new_state((18, 129, 129), EDGES2, 1)
    with ReweightedArrival(pm, names, THR) as A, ReweightedHistogram(pm, ['late'], None, edges=EDGES2) as H, \
            ArrivalMaps(pm, THR) as B:
        assert A.days == days and A.N == 129 and H.days == days
        for m, (mem, w) in enumerate(zip(MEMBERS, WEIGHTS)):
            _evaluate(pm, mem)
            A.add(_lams(names, m), w)
            H.add([LAM['late'][m]], w)
            B.add(w)
            f = _fields(pm, days)
            WA.add(sa, f, _lams(names, m), w)
            WH.add(sh, f, [LAM['late'][m]], w)
        _check_arr(A, sa, names, levels=(0.3, 0.95))
        _check_hist(H, sh, ['late'], days, levels=(0.5,))
        assert A.plane('swing', 1, 17).max() > 0 or A.plane('swing', 0, 17).max() > 0
        for k in range(2):
            assert np.array_equal(A.quantile('flat', k, 0.5), B.quantile(k, 0.5))
            for d in (0, 9, 17):
                assert np.array_equal(A.prob_by('flat', k, d), B.prob_by(k, d)), (k, d)
    pm.close()


def _hist_maps(H, names, keys, levels=(0.5, 0.95)):
    out = {}
    for n in names:
        for d in keys:
            for b in range(1, H.edges.size + 1):
                out[n, d, b] = H.plane(n, d, b)
            for p in levels:
                out[n, d, 'q', p] = H.quantile(n, d, p)[0]
    return out


def _arr_maps(A, names, levels=(0.5, 0.95)):
    out = {}
    for n in names:
        for k in range(len(A.thresholds)):
            for d in A.days:
                out[n, k, d] = A.plane(n, k, d)
                out[n, k, d, 'p'] = A.prob_by(n, k, d)
            for p in levels:
                out[n, k, 'q', p] = A.quantile(n, k, p)
    return out


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def _close_planes(X, Y, names, planes, rtol=1e-12):
    """two handles within the merge tolerance of test_reweight_gpu._check_close: the total weights to 1e-14, every
    plane as a share of its scenario's weight to rtol (atol rtol 1e-3, as the exceedance there)"""
    for n in names:
        assert abs(X.log_total_weight(n) - Y.log_total_weight(n)) <= 1e-14 * max(1.0, abs(Y.log_total_weight(n)))
        wx, wy = X.total_weight(n), Y.total_weight(n)
        for key in planes:
            np.testing.assert_allclose(X.plane(n, *key) / wx, Y.plane(n, *key) / wy, rtol=rtol, atol=rtol * 1e-3)


def test_add_order_and_merge_order():
    from parasitoids_amd.predictive import ReweightedArrival, ReweightedHistogram, ReweightedSummary
    pm = _pop_model()
    days = [0, 2, 5]
    hs = [ReweightedHistogram(pm, NAMES, days, edges=EDGES9) for _ in range(7)]
    as_ = [ReweightedArrival(pm, NAMES, THR, days) for _ in range(7)]
    ss = [ReweightedSummary(pm, NAMES, days, [1.0, 10.0]) for _ in range(3)]       # the exceedance at edges 4 and 5
    for m, (mem, w) in enumerate(zip(MEMBERS, WEIGHTS)):
        _evaluate(pm, mem)
        lam = _lams(NAMES, m)
        for group in (hs, as_):
            one, a1, b1, a2, b2, empty, rev = group
            one.add(lam, w)
            for h in ((a1, a2) if m < 2 else (b1, b2)):
                h.add(lam, w)
        ss[0].add(lam, w)
        ss[1 if m < 2 else 2].add(lam, w)
    for m in reversed(range(len(MEMBERS))):
        _evaluate(pm, MEMBERS[m])
        hs[6].add(_lams(NAMES, m), WEIGHTS[m])
        as_[6].add(_lams(NAMES, m), WEIGHTS[m])
    ss[1].merge(ss[2])
    hplanes = [(d, b) for d in days for b in range(1, 10)]
    aplanes = [(k, d) for k in range(2) for d in days]
    for group, maps, planes in ((hs, lambda h: _hist_maps(h, NAMES, days), hplanes),
                                (as_, lambda h: _arr_maps(h, NAMES), aplanes)):
        one, a1, b1, a2, b2, empty, rev = group
        assert a1.ref == [0.0, 0.0, 0.5] and b1.ref == [0.0, 2.25, 3.0]     # the two sides sit on different scales
        before = maps(b1)
        info = [(b1.members(n), b1.skipped(n), b1.log_total_weight(n)) for n in NAMES]
        empty.merge(b1)                                    # into an empty handle: a copy, bit for bit
        assert _same(maps(empty), before) and empty.ref == b1.ref
        assert [(empty.members(n), empty.skipped(n), empty.log_total_weight(n)) for n in NAMES] == info
        a1.merge(b1)
        assert _same(maps(b1), before)                     # src is unchanged
        assert [(b1.members(n), b1.skipped(n), b1.log_total_weight(n)) for n in NAMES] == info
        b2.merge(a2)                                       # the other order
        for h in (a1, b2, rev):
            assert h.ref == one.ref
            _close_planes(h, one, NAMES, planes)
        for h in (a1, b2):
            assert [(h.members(n), h.skipped(n)) for n in NAMES] == [(one.members(n), one.skipped(n)) for n in NAMES]
        # the same merge as the ReweightedSummary's: the host side bit for bit
        assert [a1.total_weight(n) for n in NAMES] == [ss[1].total_weight(n) for n in NAMES] and a1.ref == ss[1].ref
        assert [rev.members(n) for n in NAMES] == [5, 5, 4]       # -800 comes first there: a member, rescaled away later
    # the merged readings against the one-handle ones, by test_reweight_gpu._check_close on the exceedances
    one, a1 = hs[0], hs[1]
    for n in NAMES:
        for d in days:
            for k, e in ((0, 4), (1, 5)):
                np.testing.assert_allclose(a1.exceed(n, d, e), ss[1].exceedance(n, d, k), rtol=1e-12, atol=1e-15)
                np.testing.assert_allclose(a1.exceed(n, d, e), one.exceed(n, d, e), rtol=1e-12, atol=1e-15)
    _check_close(ss[1], ss[0], NAMES, days)
    assert as_[1].member_log_weights('swing') == as_[0].member_log_weights('swing')      # a1 then b1: the add order
    with ReweightedHistogram(pm, NAMES, [0, 2, 4], edges=EDGES9) as other:
        with pytest.raises(ValueError, match='different days'):
            hs[0].merge(other)
    with ReweightedArrival(pm, NAMES[:2], THR, days) as other:
        with pytest.raises(ValueError, match='scenarios'):
            as_[0].merge(other)
    for h in hs + as_ + ss:
        h.close()
    pm.close()


def test_a_release_plan_and_an_emergence_projection_as_sources():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import (ArrivalMaps, Projection, ReleaseSites, ReweightedArrival,
                                            ReweightedHistogram, SpreadHistogram, emergence_plan, lagged_models)
    pm = _pop_model()
    res = 10000.0 / 128
    late = lagged_models(pm, [0, 2])
    plan = [(0.0, 0.0, 0.6, 0), (13 * res, 6 * res, 0.4, 2)]
    W, in_days, labels = emergence_plan(dict(collection_day=5, obs_days=[24, 27]), 6)
    names = ['swing', 'late', 'flat']
    out_days = [0, 2, 3, 5]
    with Projection(pm, W, in_days) as P, ReleaseSites(pm, plan, out_days, late) as RS, \
            ReweightedHistogram.for_projection(P, names, edges=EDGES9) as HP_, \
            ReweightedArrival.for_projection(P, names, THR[:1]) as AP, \
            ReweightedHistogram.for_projection(RS, names, edges=EDGES9) as HS, \
            ReweightedArrival.for_projection(RS, names, THR) as AS, \
            SpreadHistogram.for_projection(RS, edges=EDGES9) as G, ArrivalMaps.for_projection(RS, THR) as B:
        lib = HS._lib
        one = L.f64([1.0, 1.0, 1.0])
        assert lib.ps_whist_add_project(HP_._h, P._h, 3, L.p_f64(one), L.p_f64(one)) == L.PS_ERR_STATE   # nothing applied
        assert lib.ps_whist_add_sites(HS._h, RS._h, 3, L.p_f64(one), L.p_f64(one)) == L.PS_ERR_STATE
        assert lib.ps_warr_add_project(AP._h, P._h, 3, L.p_f64(one), L.p_f64(one)) == L.PS_ERR_STATE
        assert lib.ps_warr_add_sites(AS._h, RS._h, 3, L.p_f64(one), L.p_f64(one)) == L.PS_ERR_STATE
        assert HS.members('flat') == 0 and AS.members('flat') == 0
        assert HP_.days == [0, 1] and HS.days == [0, 1, 2, 3] and AS.days == out_days and AP.days == [0, 1]
        shp, sap = WH.new_state((2, 257, 257), EDGES9, 3), WA.new_state((2, 257, 257), THR[:1], 3)
        shs, sas = WH.new_state((4, 257, 257), EDGES9, 3), WA.new_state((4, 257, 257), THR, 3)
        for m, (mem, w) in enumerate(zip(MEMBERS, WEIGHTS)):
            _evaluate(pm, mem)
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)
                late[2].evaluate(HP, mem[0], DLP, mem[1], NPER, ndays=4, want_stats=False)
            P.apply()
            RS.apply()
            lam = _lams(names, m)
            for acc in (HP_, AP, HS, AS):
                acc.add(lam, w)
            G.add(w)
            B.add(w)
            fp = np.array([P.field(k) for k in range(2)])
            fs = np.array([RS.field(k) for k in range(4)])
            WH.add(shp, fp, lam, w)
            WA.add(sap, fp, lam, w)
            WH.add(shs, fs, lam, w)
            WA.add(sas, fs, lam, w)
        _check_hist(HP_, shp, names, [0, 1], levels=(0.5, 0.95))
        _check_arr(AP, sap, names, levels=(0.5,))
        _check_hist(HS, shs, names, [0, 1, 2, 3], levels=(0.5, 0.95))
        _check_arr(AS, sas, names, levels=(0.5, 0.95))
        assert HS.plane('swing', 3, 5).max() > 0 and AS.plane('late', 0, 5).max() > 0
        for e, d in enumerate(out_days):
            assert np.array_equal(HS.quantile('flat', e, 0.5)[0], G.quantile(e, 0.5))
            assert np.array_equal(AS.prob_by('flat', 1, d), B.prob_by(1, d))
        assert [c['quantiles'] for c in AS.reached_area('flat', 0, B)] == [c['quantiles'] for c in B.reached_area(0)]
    for m in (pm, late[2]):
        m.close()


def test_refusals_change_nothing():
    import ctypes as C
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import ReweightedArrival, ReweightedHistogram
    pm = _pop_model()
    small = _pop_model(R=64)
    days = [0, 3, 5]
    for cls, tail in ((ReweightedHistogram, (days,)), (ReweightedArrival, (THR, days))):
        for bad in (['a', 'b', 'c', 'd', 'e'], ['a', 'a'], [], 'ab'):
            with pytest.raises(ValueError, match='scenario'):
                cls(pm, bad, *tail)
    for edges in ([10.0, 1.0], [1.0], [0.0, 1.0], [1.0, INF]):
        with pytest.raises(ValueError):
            ReweightedHistogram(pm, NAMES, days, edges=edges)
    for thr in ([10.0, 1.0], [1.0, 1.0], [0.0, 1.0], [], [1, 2, 3, 4, 5]):
        with pytest.raises(ValueError):
            ReweightedArrival(pm, NAMES, thr, days)
    lib = L.load()
    h = L._VP()
    e2 = L.f64(EDGES2)
    for nscen, nslot, nedge in ((0, 3, 2), (5, 3, 2), (2, 0, 2), (2, 33, 2), (2, 3, 1), (2, 3, 1025)):
        assert lib.ps_whist_create(0, 257, nscen, nslot, nedge, L.p_f64(e2), C.byref(h)) == L.PS_ERR_BAD_ARG
    assert lib.ps_whist_create(0, 257, 2, 3, 2, L.p_f64(L.f64([10.0, 1.0])), C.byref(h)) == L.PS_ERR_BAD_ARG
    for nscen, nslot, nthr in ((0, 3, 2), (5, 3, 2), (2, 0, 2), (2, 33, 2), (2, 3, 0), (2, 3, 5)):
        assert lib.ps_warr_create(0, 257, nscen, nslot, nthr, L.p_f64(e2), C.byref(h)) == L.PS_ERR_BAD_ARG
    # a histogram that does not fit names its bytes: 4 scenarios x 32 days x 1024 edges at R = 400 are 673 GB
    big = types.SimpleNamespace(days=list(range(32)), rad_res=400, rad_dist=10000.0, device=0)
    with pytest.raises(ValueError, match=r'x 8 B = 672 GB do not fit'):
        ReweightedHistogram(big, ['a', 'b', 'c', 'd'], None, bins=(1e-8, 1e6, 73))
    with ReweightedHistogram(pm, NAMES, days, edges=EDGES9) as H, ReweightedArrival(pm, NAMES, THR, days) as A:
        for R in (H, A):
            with pytest.raises(ValueError, match='last evaluation'):
                R.add([0.0, 0.0, 0.0])                   # nothing evaluated yet
        _evaluate(pm, MEMBERS[0])
        _evaluate(small, MEMBERS[0])
        for R in (H, A):
            R.add(_lams(NAMES, 0), 1)
        _evaluate(pm, MEMBERS[1])
        for R in (H, A):
            R.add([0.0, -1.5, -INF], 3)
        # 9: W = 0, a wrong scenario, a day outside the handle
        for call in (lambda: H.quantile('late', 3, 0.5), lambda: H.exceed('late', 3, 0),
                     lambda: A.prob_by('late', 0, 3), lambda: A.quantile('late', 0, 0.5)):
            with pytest.raises(L.HipError) as err:
                call()
            assert err.value.code == L.PS_ERR_STATE
        assert not H.plane('late', 3, 5).any() and not A.plane('late', 0, 3).any()    # a raw plane of zeros is read
        for call in (lambda: H.quantile('trap', 3, 0.5), lambda: H.exceed('trap', 3, 0), lambda: H.plane('trap', 3, 1),
                     lambda: A.prob_by('trap', 0, 3), lambda: A.quantile('trap', 0, 0.5),
                     lambda: A.reached_area('trap', 0, None)):
            with pytest.raises(ValueError, match='not one of'):
                call()
        for d in (1, 2, 4, 6):
            with pytest.raises(ValueError, match='not in the reweighted histogram'):
                H.quantile('swing', d, 0.5)
            with pytest.raises(ValueError, match='not in the reweighted arrival maps'):
                A.prob_by('swing', 0, d)
        for call in (lambda: H.exceed('swing', 3, 9), lambda: H.plane('swing', 3, 0), lambda: H.plane('swing', 3, 10),
                     lambda: A.prob_by('swing', 2, 3), lambda: H.quantile('swing', 3, 0.0),
                     lambda: A.quantile('swing', 0, 1.5)):
            with pytest.raises(ValueError):
                call()
        names = NAMES[:2]
        before = _hist_maps(H, names, days), _arr_maps(A, names)
        host = [[(R.members(n), R.skipped(n), R.log_total_weight(n)) for n in NAMES] + list(R.ref) for R in (H, A)]
        rows = A.member_log_weights('swing')
        for R in (H, A):
            for lam in ([0.0, math.nan, 0.0], [INF, 0.0, 0.0], [0.0, 0.0], [0.0] * 4, 'abc', {'flat': 0.0}):
                with pytest.raises(ValueError):
                    R.add(lam)
            for w in (0, -1, math.nan, INF):
                with pytest.raises(ValueError, match='weight'):
                    R.add([0.0, 0.0, 0.0], w)
        # the library's own checks: every argument before anything is enqueued
        kind, idx, delta = H._kind, H._idx, H._delta
        stat, post = L.f64([130000.0, 1.0, 1.0]), L.f64([1.0, 130000.0, 130000.0])

        def add(fn, R, solver, nslot, nscen, r, om, idx=idx):
            return fn(R._h, solver._h, nslot, L.p_i32(kind), L.p_i32(idx), L.p_f64(stat), L.p_f64(post),
                      L.p_i32(delta), 1e-8, nscen, L.p_f64(L.f64(r)), L.p_f64(L.f64(om)))
        ok = [1.0, 1.0, 1.0]
        for fn, R in ((lib.ps_whist_add, H), (lib.ps_warr_add, A)):
            assert add(fn, R, small.solver, 3, 3, ok, ok) == L.PS_ERR_BAD_ARG and b'domain' in lib.ps_last_error()
            assert add(fn, R, pm.solver, 2, 3, ok, ok) == L.PS_ERR_BAD_ARG
            assert add(fn, R, pm.solver, 3, 2, ok, ok) == L.PS_ERR_BAD_ARG
            assert add(fn, R, pm.solver, 3, 4, ok + [1.0], ok + [1.0]) == L.PS_ERR_BAD_ARG
            for om in ([1.0, math.nan, 1.0], [1.0, 1.0, -0.5], [INF, 1.0, 1.0]):
                assert add(fn, R, pm.solver, 3, 3, ok, om) == L.PS_ERR_BAD_ARG and b'omega' in lib.ps_last_error()
            for r in ([1.5, 1.0, 1.0], [1.0, -0.1, 1.0], [1.0, 1.0, math.nan]):
                assert add(fn, R, pm.solver, 3, 3, r, ok) == L.PS_ERR_BAD_ARG and b'rescale' in lib.ps_last_error()
            assert add(fn, R, pm.solver, 3, 3, ok, ok, idx=L.i32([0, 2, 9])) != L.PS_OK   # chain record 9 of a 6-day run
        buf = np.empty((257, 257))
        assert lib.ps_whist_fetch(H._h, 3, 0, 1, L.p_f64(buf)) == L.PS_ERR_BAD_ARG
        assert lib.ps_whist_fetch(H._h, 0, 3, 1, L.p_f64(buf)) == L.PS_ERR_BAD_ARG
        assert lib.ps_whist_fetch(H._h, 0, 0, 10, L.p_f64(buf)) == L.PS_ERR_BAD_ARG
        assert lib.ps_warr_fetch(A._h, 0, 2, 0, L.p_f64(buf)) == L.PS_ERR_BAD_ARG
        assert lib.ps_warr_fetch(A._h, 0, 0, 3, L.p_f64(buf)) == L.PS_ERR_BAD_ARG
        assert lib.ps_whist_merge(H._h, H._h, L.p_f64(L.f64(ok)), L.p_f64(L.f64(ok))) == L.PS_ERR_BAD_ARG
        assert lib.ps_warr_merge(A._h, A._h, L.p_f64(L.f64(ok)), L.p_f64(L.f64(ok))) == L.PS_ERR_BAD_ARG
        with ReweightedHistogram(pm, NAMES, days, edges=EDGES2) as other:
            assert lib.ps_whist_merge(H._h, other._h, L.p_f64(L.f64(ok)), L.p_f64(L.f64(ok))) == L.PS_ERR_BAD_ARG
        with ReweightedArrival(small, NAMES, THR, days) as other:
            assert lib.ps_warr_merge(A._h, other._h, L.p_f64(L.f64(ok)), L.p_f64(L.f64(ok))) == L.PS_ERR_BAD_ARG
        # after all of them every plane and the host side are bit for bit what they were
        assert _same(_hist_maps(H, names, days), before[0]) and _same(_arr_maps(A, names), before[1])
        assert [[(R.members(n), R.skipped(n), R.log_total_weight(n)) for n in NAMES] + list(R.ref) for R in (H, A)] == host
        assert A.member_log_weights('swing') == rows
    pm.close()
    small.close()


def _npz_equal(a, b):
    fa, fb = np.load(a), np.load(b)
    return sorted(fa.files) == sorted(fb.files) and all(np.array_equal(fa[k], fb[k]) for k in fa.files)


def test_posterior_predictive_with_the_maps_option(tmp_path):
    from parasitoids_amd import predictive as PR
    N = 257
    res_m = 10000.0 / 128
    trace, names = _chain([3, 2, 4, 3])
    chain = (trace, names)
    rng = np.random.default_rng(4)
    tilt = np.repeat([0.0, 1.5, -0.75, 2.5], [3, 2, 4, 3]) + 0.01 * rng.normal(size=12)
    rw = {'tilt': dict(log_weights=[tilt]), 'flat': dict(log_weights=[np.zeros(12)])}
    out = [0, 2, 3, 5]
    kw = dict(thresholds=THR, quantiles=[0.05, 0.5], edges=EDGES9, arrival=THR, arrival_levels=(0.5, 0.95),
              sites=dict(sites=[(0.0, 0.0, 0.6), (13 * res_m, 6 * res_m, 0.5, 2)], days=out),
              exposure=[2, 4])
    pm = _pop_model(mode='exact')       # an auto-mode model routes days by what it has seen
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        plain = PR.posterior_predictive(pm, chain, reweight=dict(rw), **kw)
        res = PR.posterior_predictive(pm, chain, reweight=dict(rw, options=dict(maps=('quantiles', 'arrival'))), **kw)
        only = PR.posterior_predictive(pm, chain, reweight=dict(rw, options=dict(maps=['arrival'])), days=[1, 3],
                                       arrival=THR)
    assert plain.reweight_histogram is None and plain.reweight_arrival is None and 'maps' not in plain.reweight_info
    assert plain.sites.reweight_histogram is None and plain.exposure.reweight_histogram is None
    assert only.reweight_histogram is None and only.reweight_arrival.days == [1, 3]
    RH, RA, S = res.reweight_histogram, res.reweight_arrival, res.summary
    assert res.reweight_info['maps'] == ['quantiles', 'arrival']
    assert RH.scenarios == RA.scenarios == ['tilt', 'flat'] and RH.days == RA.days == S.days == list(range(6))
    assert np.array_equal(RH.edges, res.histogram.edges) and RA.thresholds == res.arrival.thresholds == THR
    for R in (RH, RA):
        assert R.ref == res.reweight.ref
        for n in ('tilt', 'flat'):
            assert (R.total_weight(n), R.members(n), R.skipped(n)) == \
                (res.reweight.total_weight(n), res.reweight.members(n), res.reweight.skipped(n))
    for d in S.days:
        assert np.array_equal(RH.quantile('flat', d, 0.5)[0], res.histogram.quantile(d, 0.5))
        assert np.array_equal(RA.prob_by('flat', 1, d), res.arrival.prob_by(1, d))
    assert not np.array_equal(RH.quantile('tilt', 5, 0.5)[0], RH.quantile('flat', 5, 0.5)[0])
    ps = res.sites
    assert ps.reweight_histogram.days == [0, 1, 2, 3] and ps.reweight_arrival.days == out
    assert res.exposure.reweight_histogram is not None and res.exposure.reweight_arrival is None
    for e in range(4):
        assert np.array_equal(ps.reweight_histogram.quantile('flat', e, 0.05)[0], ps.histogram.quantile(e, 0.05))
    assert np.array_equal(ps.reweight_arrival.quantile('flat', 0, 0.5), ps.arrival.quantile(0, 0.5))
    # the files
    plain.save(str(tmp_path / 'p' / 'pp'))
    res.save(str(tmp_path / 'm' / 'pp'))
    new = ['pp_exposure_reweight_quantiles.npz', 'pp_reweight_arrival.npz', 'pp_reweight_quantiles.npz',
           'pp_sites_reweight_arrival.npz', 'pp_sites_reweight_quantiles.npz']
    old = sorted(os.listdir(str(tmp_path / 'p')))
    assert sorted(os.listdir(str(tmp_path / 'm'))) == sorted(old + new) and not set(old) & set(new)
    for name in old:                                   # every file the option does not name holds what it held
        if name.endswith('.npz'):
            assert _npz_equal(str(tmp_path / 'p' / name), str(tmp_path / 'm' / name)), name
    jp = json.load(open(str(tmp_path / 'p' / 'pp.json')))
    jm = json.load(open(str(tmp_path / 'm' / 'pp.json')))
    assert 'maps' not in jp['predictive']['reweight'] and 'reached_area' not in jp['predictive']['reweight']
    assert 'reweight' not in jp['predictive']['sites']
    meta = jm['predictive']['reweight']
    assert meta.pop('maps') == ['quantiles', 'arrival']
    curve = meta.pop('reached_area')
    assert jm['predictive']['sites'].pop('reweight')['reached_area'].keys() == {'tilt', 'flat'}
    assert jm == jp                                    # but for the new keys the json is what it was
    assert curve['flat'] == jm['predictive']['arrival']['reached_area']
    assert curve['tilt'] != curve['flat'] and len(curve['tilt']) == 2 and len(curve['tilt'][0]) == 6
    labels = [pm.days[d] for d in S.days]
    f = np.load(str(tmp_path / 'm' / 'pp_reweight_quantiles.npz'))
    assert [str(n) for n in f['scenarios']] == ['tilt', 'flat'] and [str(x) for x in f['labels']] == [str(x) for x in labels]
    for j, n in enumerate(['tilt', 'flat']):
        for d, label in zip(S.days, labels):
            for p, tag in ((0.05, 'q5'), (0.5, 'q50')):
                m = RH.quantile(n, d, p)[0]
                assert np.array_equal(_csr(f, 's%d_%s_%s' % (j, label, tag), N), np.where(m >= 1e-8, m, 0.0))
    f = np.load(str(tmp_path / 'm' / 'pp_reweight_arrival.npz'))
    for j, n in enumerate(['tilt', 'flat']):
        for k in range(2):
            for d, label in zip(S.days, labels):
                m = RA.prob_by(n, k, d)
                assert np.array_equal(_csr(f, 's%d_%s_parr%d' % (j, label, k), N), np.where(m >= 1e-8, m, 0.0))
            for p, tag in ((0.5, 'q50'), (0.95, 'q95')):
                got = f['s%d_arrival%d_%s' % (j, k, tag)]
                assert got.dtype == np.int16 and np.array_equal(got, RA.quantile(n, k, p))
    f = np.load(str(tmp_path / 'm' / 'pp_sites_reweight_arrival.npz'))
    m = ps.reweight_arrival.prob_by('tilt', 0, 3)
    assert np.array_equal(_csr(f, 's0_3_parr0', N), np.where(m >= 1e-8, m, 0.0))
    f = np.load(str(tmp_path / 'm' / 'pp_sites_reweight_quantiles.npz'))
    m = ps.reweight_histogram.quantile('tilt', 3, 0.5)[0]
    assert np.array_equal(_csr(f, 's0_5_q50', N), np.where(m >= 1e-8, m, 0.0))
    pm.close()
