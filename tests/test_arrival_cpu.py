"""CPU tests of the posterior arrival maps (predictive.ArrivalMaps, ps_arrival_*): the numpy reference on
hand-made fields (first arrival kept, ties, never, monotone in k, quantile boundaries, weighted areas),
argument checks before any evaluation, the result file with and without arrival maps, and no maps without a
device."""
import json
import types

import numpy as np
import pytest

from parasitoids_amd import predictive as PP

from arrival_ref import (area_quantile, arrival_slots, cumulative, probability, quantile_slots, reached_rows,
                         weighted_counts)


def _member(*cols):
    """[nslot, ncell] from one value list per cell"""
    return np.array(cols, dtype=np.float64).T


# ------------------------------------------------------------------ the numpy reference, by hand
def test_rise_and_fall_keeps_the_first_arrival():
    f = _member([0.0, 2.0, 0.5, 3.0, 0.1])          # one cell: above 1 on slot 1, below, above again
    a = arrival_slots(f, [1.0, 2.5])
    assert a[:, 0].tolist() == [1, 3]
    assert reached_rows([f], [1.0, 2.5])[0].tolist() == [[0, 1, 1, 1, 1], [0, 0, 0, 1, 1]]


def test_value_equal_to_the_threshold_counts_as_arrived():
    f = _member([0.0, 1.0, 0.0], [0.0, 0.999999, 0.0])
    assert arrival_slots(f, [1.0])[0].tolist() == [1, 3]


def test_zero_cells_and_cells_that_never_arrive():
    f = _member([0.0] * 4, [0.5] * 4, [9.0, 0.0, 0.0, 0.0])
    c = weighted_counts([f, f], [2, 3], [1.0, 10.0])
    assert c.shape == (2, 5, 3)
    assert c[0, 4].tolist() == [5, 5, 0] and c[0, 0].tolist() == [0, 0, 5]
    assert c[1, 4].tolist() == [5, 5, 5] and c[1, :4].sum() == 0
    P = probability(c)
    assert P[0, :, 2].tolist() == [1.0] * 4 and P[0, :, :2].sum() == 0.0 and P[1].sum() == 0.0


def test_arrival_is_monotone_in_k():
    rng = np.random.default_rng(3)
    f = 10 ** rng.uniform(-3, 2, size=(6, 400))
    f[rng.random(f.shape) < 0.3] = 0.0
    thr = [0.01, 0.5, 3.0, 40.0]
    a = arrival_slots(f, thr)
    assert np.all(np.diff(a, axis=0) >= 0)
    members = [f, f[::-1].copy(), np.roll(f, 1, axis=0)]
    P = probability(weighted_counts(members, [1, 2, 4], thr))
    assert np.all(np.diff(P, axis=0) <= 0) and np.all(np.diff(P, axis=1) >= 0)
    rows = reached_rows(members, thr)
    assert np.all(np.diff(rows, axis=1) <= 0) and np.all(np.diff(rows, axis=2) >= 0)


def test_quantiles_at_the_boundary_at_one_and_beyond_the_window():
    # one cell, W = 10: 4 arrive on slot 0, 1 on slot 2, 5 never
    members = [_member([5.0, 5.0, 5.0]), _member([0.0, 0.0, 2.0]), _member([0.0, 0.0, 0.0])]
    w = [4, 1, 5]
    c = weighted_counts(members, w, [1.0])
    assert c[0, :, 0].tolist() == [4, 0, 1, 5]
    assert cumulative(c)[0, :, 0].tolist() == [4, 4, 5]
    assert quantile_slots(c, 0.4)[0, 0] == 0          # C = 4 == 0.4 W exactly: arrived
    assert quantile_slots(c, 0.41)[0, 0] == 2
    assert quantile_slots(c, 0.5)[0, 0] == 2          # C = 5 == 0.5 W
    assert quantile_slots(c, 0.51)[0, 0] == -1        # beyond the window
    assert quantile_slots(c, 1.0)[0, 0] == -1
    everyone = weighted_counts(members[:2], w[:2], [1.0])
    assert quantile_slots(everyone, 1.0)[0, 0] == 2    # p = 1: the slot where the last member arrives
    assert probability(c)[0, :, 0].tolist() == [0.4, 0.4, 0.5]


def test_weighted_area_quantiles():
    n = np.array([10, 3, 7, 3])
    w = np.array([1, 2, 3, 4])                          # sorted: 3 (w 6), 7 (w 3), 10 (w 1); W = 10
    assert area_quantile(n, w, 0.6) == 3 and area_quantile(n, w, 0.61) == 7
    assert area_quantile(n, w, 0.9) == 7 and area_quantile(n, w, 0.91) == 10 and area_quantile(n, w, 1.0) == 10
    for p in (0.05, 0.6, 0.61, 0.9, 0.95, 1.0):
        assert PP.weighted_lower_quantile(n, w, p) == area_quantile(n, w, p), p


# ------------------------------------------------------------------ argument checks
def test_threshold_and_day_checks():
    assert PP.check_arrival_thresholds((1, 10)) == [1.0, 10.0]
    assert PP.check_arrival_days(range(32)) == list(range(32))
    for bad in ([], [10, 1], [1, 1], [0, 1], [-1], [1, float('nan')], [1, float('inf')], [1, 2, 3, 4, 5]):
        with pytest.raises(ValueError):
            PP.check_arrival_thresholds(bad)
    for bad in ([], [2, 1], [0, 0], [-1, 2], list(range(33))):
        with pytest.raises(ValueError):
            PP.check_arrival_days(bad)


def _chain():
    from parasitoids_amd import mcmc
    names = [m[0] for m in mcmc.MODEL_BLOCK]
    t0 = np.array([m[2] for m in mcmc.MODEL_BLOCK])
    return np.array([t0, t0, t0 * 1.01]), names


@pytest.mark.parametrize('kw', [dict(arrival=[10, 1]), dict(arrival=[1, 1]), dict(arrival=[0, 1]),
                                dict(arrival=[-2.0]), dict(arrival=[1, float('nan')]), dict(arrival=[1, 2, 3, 4, 5]),
                                dict(arrival=[]), dict(arrival=[1], days=[2, 0, 5]), dict(arrival=[1], days=[1, 1]),
                                dict(arrival=[1], arrival_levels=[0.0]), dict(arrival=[1], arrival_levels=[1.5]),
                                dict(arrival=[1], arrival_levels=[0.5, float('nan')])])
def test_bad_arrival_arguments_raise_before_any_evaluation(kw):
    calls = []

    def evaluate(theta):
        calls.append(theta)
        return True
    with pytest.raises(ValueError):
        PP.posterior_predictive(None, _chain(), evaluate=evaluate, **kw)
    assert calls == []


def test_no_device_gives_no_arrival_maps():
    res = PP.posterior_predictive(None, _chain(), arrival=[1.0, 10.0], evaluate=lambda theta: True)
    assert res.summary is None and res.arrival is None
    res = PP.posterior_predictive(None, _chain(), evaluate=lambda theta: True)
    assert res.arrival is None and res.arrival_levels is None


# ------------------------------------------------------------------ result files
class _Summary():
    def __init__(self, days):
        self.days = days
        self.pm = types.SimpleNamespace(days=[100 + d for d in range(max(days) + 1)])
        self.thresholds = [1.0]
        self.total_weight = 3.0
        self.members = 2

    def mean(self, d):
        return np.full((5, 5), 10.0 + d)

    def sd(self, d):
        return np.full((5, 5), 1.0)

    def exceedance(self, d, k):
        return np.eye(5)


class _Arrival():
    """what save() uses of ArrivalMaps, from numpy reference counts of two 5 x 5 members"""
    thresholds = [1.0, 10.0]
    cell_area = 625.0

    def __init__(self, days):
        self.days = days
        a = np.zeros((len(days), 5, 5))
        a[0, 2, 2] = 20.0           # arrives on the first day at both thresholds
        a[1:, 2, 1:4] = 5.0
        b = np.zeros((len(days), 5, 5))
        b[1:, 0, 0] = 1.0
        self.members = [a, b]
        self.w = [1, 2]
        self.c = weighted_counts(self.members, self.w, self.thresholds)

    def prob_by(self, k, d):
        return probability(self.c)[k, self.days.index(d)]

    def quantile(self, k, p):
        s = quantile_slots(self.c, p)[k]
        return np.where(s < 0, -1, np.asarray(self.days)[s.clip(0)]).astype(np.int32)

    def reached(self, k):
        return reached_rows(self.members, self.thresholds)[:, k, :], np.array(self.w, dtype=np.int64)

    def reached_area(self, k, levels):
        return PP.ArrivalMaps.reached_area(self, k, levels)


def _old_keys(days):
    keys = {'days'}
    for d in days:
        for suffix in ('', '_sd', '_pexc0'):
            keys |= {'%d%s_%s' % (100 + d, suffix, t) for t in ('data', 'ind', 'indptr')}
    return keys


def test_save_with_arrival_maps_adds_exactly_the_new_keys(tmp_path):
    days = [0, 2, 3]
    A = _Arrival(days)
    res = PP.PredictiveResult(_Summary(days), 3, 2, 0, 0.1, [], None, [], days, arrival=A,
                              arrival_levels=[0.05, 0.5, 0.95])
    npz, js = res.save(str(tmp_path / 'pp'))
    new = {'%d_parr%d_%s' % (100 + d, k, t) for d in days for k in (0, 1) for t in ('data', 'ind', 'indptr')}
    new |= {'arrival%d_%s' % (k, q) for k in (0, 1) for q in ('q5', 'q50', 'q95')}
    new |= {'arrival0_cells', 'arrival1_cells', 'arrival_weights'}
    with np.load(npz) as f:
        assert set(f.files) == _old_keys(days) | new
        q = f['arrival0_q5']
        assert q.dtype == np.int16 and q.shape == (5, 5)
        assert q[2, 2] == 0 and q[2, 1] == 2 and q[4, 4] == -1     # a day-0 arrival survives (dense)
        assert np.array_equal(f['arrival1_q50'], A.quantile(1, 0.5))
        assert f['arrival0_cells'].tolist() == [[1, 3, 3], [0, 1, 1]]
        assert f['arrival1_cells'].tolist() == [[1, 1, 1], [0, 0, 0]]
        assert f['arrival_weights'].tolist() == [1, 2]
        from scipy import sparse
        M = sparse.csr_matrix((f['102_parr0_data'], f['102_parr0_ind'], f['102_parr0_indptr']), shape=(5, 5))
        assert np.array_equal(M.toarray(), A.prob_by(0, 2))
    meta = json.load(open(js))
    a = meta['predictive']['arrival']
    assert a['thresholds'] == [1.0, 10.0] and a['levels'] == [0.05, 0.5, 0.95] and a['days'] == days
    assert a['cell_area'] == 625.0
    ra = a['reached_area']
    assert len(ra) == 2 and [r['day'] for r in ra[0]] == days
    # threshold 0, day 2: member areas 3 (w 1) and 1 (w 2) cells
    r = ra[0][1]
    assert r['mean'] == (3 * 1 + 1 * 2) / 3 * 625.0
    assert r['quantiles'] == [625.0, 625.0, 3 * 625.0]
    assert r['radius_quantiles'] == [float(np.sqrt(q / np.pi)) for q in r['quantiles']]
    assert r['radius_mean'] == float(np.sqrt(r['mean'] / np.pi))


def test_save_without_arrival_maps_writes_todays_keys(tmp_path):
    res = PP.PredictiveResult(_Summary([0, 2]), 3, 2, 0, 0.1, [], None, [], [0, 2])
    assert res.arrival is None and res.arrival_levels is None
    npz, js = res.save(str(tmp_path / 'pp'))
    with np.load(npz) as f:
        assert set(f.files) == _old_keys([0, 2])
    meta = json.load(open(js))
    assert 'arrival' not in meta['predictive']
