"""CPU tests of the posterior peak maps (predictive.PeakMaps, ps_peak_*): the numpy reference on hand-made and
random fields (the first of two equal maxima wins, all-zero cells, a cell above the top threshold throughout,
the identities between counts, durations and exceedances, the quantile rule at its boundaries), and the argument
checks of PeakMaps and of posterior_predictive(peak=...) before any evaluation, and the result file of save_peak."""
import types

import numpy as np
import pytest

from parasitoids_amd import predictive as PP

import peak_ref as R


def _member(*cols):
    """[nslot, ncell] from one value list per cell"""
    return np.array(cols, dtype=np.float64).T


# ------------------------------------------------------------------ the numpy reference, by hand
def test_the_first_of_two_equal_maxima_wins():
    f = _member([0.0, 4.0, 1.0, 4.0, 0.5], [2.0, 2.0, 2.0, 2.0, 2.0], [0.0, 0.0, 0.0, 0.0, 7.0])
    assert R.peak_field(f).tolist() == [4.0, 2.0, 7.0]
    assert R.peak_slot(f).tolist() == [1, 0, 4]
    assert R.durations(f, [1.0, 4.0]).tolist() == [[3, 5, 1], [2, 0, 1]]      # >= : 4.0 counts at t = 4


def test_all_zero_cells_have_no_peak_day_and_duration_zero():
    f = _member([0.0] * 4, [0.0, 0.0, 3.0, 0.0])
    assert R.peak_slot(f).tolist() == [4, 2] and R.peak_field(f).tolist() == [0.0, 3.0]
    dc = R.day_counts([f, f], [2, 3])
    assert dc[:, 0].tolist() == [0, 0, 0, 0, 5] and dc[:, 1].tolist() == [0, 0, 5, 0, 0]
    uc = R.duration_counts([f, f], [2, 3], [1.0])
    assert uc[0, :, 0].tolist() == [5, 0, 0, 0, 0] and uc[0, :, 1].tolist() == [0, 5, 0, 0, 0]
    assert R.day_prob(dc)[:, 0].tolist() == [0.0] * 4 and R.day_quantile(dc, 0.05)[0] == -1
    assert R.duration_quantile(uc[0], 1.0).tolist() == [0, 1]
    assert R.duration_mean(uc[0]).tolist() == [0.0, 1.0]


def test_a_cell_above_the_top_threshold_on_every_slot():
    f = _member([50.0, 60.0, 55.0], [0.5, 20.0, 0.5])
    thr = [1.0, 10.0]
    assert R.durations(f, thr).tolist() == [[3, 1], [3, 1]]
    uc = R.duration_counts([f], [4], thr)
    assert uc[1, :, 0].tolist() == [0, 0, 0, 4] and uc[1, :, 1].tolist() == [0, 4, 0, 0]
    P = R.duration_prob(uc[1])
    assert P[:, 0].tolist() == [1.0, 1.0, 1.0, 1.0] and P[:, 1].tolist() == [1.0, 1.0, 0.0, 0.0]
    assert R.duration_quantile(uc[1], 0.05).tolist() == [3, 1]


def test_counts_sum_to_the_weight_and_durations_to_the_exceedances():
    rng = np.random.default_rng(5)
    thr = [0.01, 0.5, 3.0, 40.0]
    members, weights = [], [1, 3, 2, 5]
    for _ in weights:
        f = 10 ** rng.uniform(-3, 2, size=(7, 300))
        f[rng.random(f.shape) < 0.4] = 0.0
        f[:, :20] = 0.0                                  # cells that hold nothing in any member
        members.append(f)
    W = sum(weights)
    dc = R.day_counts(members, weights)
    uc = R.duration_counts(members, weights, thr)
    assert np.all(dc.sum(0) == W) and np.all(uc.sum(1) == W)
    assert np.all(dc[-1, :20] == W) and np.all(uc[:, 0, :20] == W)
    for k, t in enumerate(thr):
        lhs = sum(n * uc[k, n] for n in range(8))
        rhs = sum(w * (f >= t).sum(0) for f, w in zip(members, weights))
        assert np.array_equal(lhs, rhs), k
        assert np.array_equal(R.duration_mean(uc[k]), lhs.astype(np.float64) / float(W))
    assert np.all(np.diff(R.day_prob(dc), axis=0) >= 0)
    assert np.all(np.diff(np.array([R.duration_prob(uc[k]) for k in range(4)]), axis=0) <= 0)   # monotone in k
    # the peak is >= every day's value, and peak >= t is the same event as some day >= t
    for f in members:
        m = R.peak_field(f)
        assert np.all(m >= f.max(0)) and np.array_equal(m, np.maximum(f.max(0), 0.0))
        assert np.array_equal(m >= thr[1], R.durations(f, thr)[1] > 0)
        p = R.peak_slot(f)
        assert np.array_equal(p == 7, m == 0.0)
        assert np.array_equal(np.where(p < 7, p, 0), np.where(p < 7, f.argmax(0), 0))   # argmax keeps the first


def test_quantiles_at_the_boundary_and_with_the_implied_zero_plane():
    # one cell, W = 10: 4 peak on slot 0, 1 on slot 2, 5 never hold anything
    members = [_member([5.0, 1.0, 1.0]), _member([0.0, 0.0, 2.0]), _member([0.0, 0.0, 0.0])]
    w = [4, 1, 5]
    dc = R.day_counts(members, w)
    assert dc[:, 0].tolist() == [4, 0, 1, 5]
    assert R.day_quantile(dc, 0.4)[0] == 0 and R.day_quantile(dc, 0.41)[0] == 2
    assert R.day_quantile(dc, 0.5)[0] == 2 and R.day_quantile(dc, 0.51)[0] == -1 and R.day_quantile(dc, 1.0)[0] == -1
    uc = R.duration_counts(members, w, [1.0])[0]
    assert uc[:, 0].tolist() == [5, 1, 0, 4]            # durations 3 (w 4), 1 (w 1), 0 (w 5)
    assert R.duration_quantile(uc, 0.5)[0] == 0 and R.duration_quantile(uc, 0.51)[0] == 1
    assert R.duration_quantile(uc, 0.6)[0] == 1 and R.duration_quantile(uc, 0.61)[0] == 3
    assert R.duration_quantile(uc, 1.0)[0] == 3
    assert R.duration_prob(uc)[:, 0].tolist() == [1.0, 0.5, 0.4, 0.4]
    assert R.duration_mean(uc)[0] == 13 / 10


# ------------------------------------------------------------------ argument checks
def test_threshold_checks_allow_an_empty_list():
    assert PP.check_peak_thresholds(()) == [] and PP.check_peak_thresholds([1, 10]) == [1.0, 10.0]
    for bad in ([10, 1], [1, 1], [0, 1], [-1], [1, float('nan')], [1, float('inf')], [1, 2, 3, 4, 5], 3.0, ['a']):
        with pytest.raises(ValueError):
            PP.check_peak_thresholds(bad)
    assert PP.check_peak([1, 10]) == ([1.0, 10.0], [0.05, 0.5, 0.95])
    assert PP.check_peak(dict(thresholds=[2], levels=(0.5,))) == ([2.0], [0.5])
    assert PP.check_peak(dict()) == ([], [0.05, 0.5, 0.95])
    for bad in (dict(thresholds=[1], level=[0.5]), dict(levels=[0.0]), dict(thresholds=[2, 1])):
        with pytest.raises(ValueError):
            PP.check_peak(bad)


@pytest.mark.parametrize('kw', [dict(thresholds=[10, 1]), dict(thresholds=[0.0]), dict(thresholds=[1, 2, 3, 4, 5]),
                                dict(thresholds=[float('nan')]), dict(days=[]), dict(days=[2, 1]), dict(days=[-1, 0]),
                                dict(days=list(range(33)))])
def test_bad_peak_maps_arguments_raise_before_the_library_is_touched(kw):
    pm = types.SimpleNamespace(days=list(range(6)))      # a stub: nothing but the day list is read before the checks
    with pytest.raises(ValueError):
        PP.PeakMaps(pm, kw.get('thresholds', [1.0]), kw.get('days'))


def test_class_attributes_make_the_peak_field_a_fields_source():
    assert PP.PeakMaps.fields_kind == 'peak' and PP.PeakMaps.nout == 1 and PP.PeakMaps.live == [0]
    from parasitoids_amd import _lib as L
    for name in ('ps_summary_add_peak', 'ps_hist_add_peak', 'ps_peak_add_project', 'ps_peak_add_sites'):
        assert name in L.SIGNATURES


def _chain():
    from parasitoids_amd import mcmc
    names = [m[0] for m in mcmc.MODEL_BLOCK]
    t0 = np.array([m[2] for m in mcmc.MODEL_BLOCK])
    return np.array([t0, t0, t0 * 1.01]), names


@pytest.mark.parametrize('kw', [dict(peak=[10, 1]), dict(peak=[1, 1]), dict(peak=[0, 1]), dict(peak=[-2.0]),
                                dict(peak=[1, float('nan')]), dict(peak=[1, 2, 3, 4, 5]),
                                dict(peak=dict(thresholds=[1], levels=[0.0])), dict(peak=dict(thresholds=[1], levels=[1.5])),
                                dict(peak=dict(threshold=[1])), dict(peak=[1], days=[2, 0, 5]), dict(peak=[1], days=[1, 1]),
                                dict(peak=[1], days=list(range(33)))])
def test_bad_peak_arguments_raise_before_any_evaluation(kw):
    with pytest.raises(ValueError) as err:
        PP.posterior_predictive(None, _chain(), **kw)     # no model either: the checks come first
    assert 'PopModel' not in str(err.value)
    with pytest.raises(ValueError, match='PopModel'):     # good arguments get as far as the missing model
        PP.posterior_predictive(None, _chain(), peak=[1, 10], days=[0, 2, 5])


def test_peak_is_refused_together_with_evaluate():
    calls = []

    def evaluate(theta):
        calls.append(theta)
        return True
    for peak in ([1.0, 10.0], [], dict(thresholds=[1.0])):
        with pytest.raises(ValueError, match='evaluate'):
            PP.posterior_predictive(None, _chain(), evaluate=evaluate, peak=peak)
    assert calls == []
    res = PP.posterior_predictive(None, _chain(), evaluate=evaluate)
    assert res.peak is None and res.summary is None


# ------------------------------------------------------------------ result files
class _Maps():
    """what save_peak uses of PeakMaps, from numpy reference counts of three 5 x 5 members"""
    thresholds = [1.0, 10.0]
    days = [0, 2, 3]
    consecutive = False
    members = 3
    total_weight = 6.0

    def __init__(self):
        rng = np.random.default_rng(1)
        members = [10 ** rng.uniform(-2, 2, size=(3, 5, 5)) * (rng.random((3, 5, 5)) > 0.4) for _ in range(3)]
        self.dc = R.day_counts(members, [1, 2, 3])
        self.uc = R.duration_counts(members, [1, 2, 3], self.thresholds)

    def day_counts(self, d):
        return self.dc[self.days.index(d)].astype(np.uint32)

    def day_quantile(self, p):
        q = R.day_quantile(self.dc, p)
        return np.where(q < 0, -1, np.asarray(self.days)[q.clip(0)]).astype(np.int32)

    def duration_counts(self, k, n):
        return self.uc[k, n].astype(np.uint32)

    def duration_quantile(self, k, p):
        return R.duration_quantile(self.uc[k], p).astype(np.int32)

    def duration_mean(self, k):
        return R.duration_mean(self.uc[k])


class _PeakSummary():
    thresholds = [1.0]

    def mean(self, e):
        return np.full((5, 5), 2.0)

    def sd(self, e):
        return np.ones((5, 5))

    def exceedance(self, e, k):
        return np.eye(5)


def test_save_peak_writes_the_listed_keys_and_the_json_block(tmp_path):
    import json
    M = _Maps()
    pk = types.SimpleNamespace(maps=M, summary=_PeakSummary(), histogram=None, levels=[0.05, 0.5])
    block = PP.save_peak(str(tmp_path / 'd' / 'pp_peak'), pk, [0.5])
    want = {'days', 'peak_thresholds', 'peak_days', 'peakday_counts', 'days0_counts', 'days1_counts'}
    want |= {'%s_%s' % (n, q) for n in ('peakday', 'days0', 'days1') for q in ('q5', 'q50')}
    want |= {'%s_%s' % (n, t) for n in ('peak', 'peak_sd', 'peak_pexc0', 'days0_mean', 'days1_mean')
             for t in ('data', 'ind', 'indptr')}
    with np.load(str(tmp_path / 'd' / 'pp_peak.npz')) as f:
        assert set(f.files) == want                          # no histogram: no peak_q{tag}
        assert f['peak_days'].tolist() == [0, 2, 3] and f['peak_thresholds'].tolist() == [1.0, 10.0]
        assert f['peakday_counts'].dtype == np.uint16 and np.array_equal(f['peakday_counts'], M.dc[:-1])
        assert np.array_equal(f['days1_counts'], M.uc[1]) and np.all(f['days1_counts'].sum(0) == 6)
        assert f['peakday_q5'].dtype == np.int16 and np.array_equal(f['peakday_q5'], M.day_quantile(0.05))
        assert np.array_equal(f['days0_q50'], M.duration_quantile(0, 0.5))
        from scipy import sparse
        D = sparse.csr_matrix((f['days0_mean_data'], f['days0_mean_ind'], f['days0_mean_indptr']), shape=(5, 5))
        assert np.array_equal(D.toarray(), M.duration_mean(0))
    assert block == {'thresholds': [1.0, 10.0], 'days': [0, 2, 3], 'levels': [0.05, 0.5], 'consecutive': False,
                     'members': 3, 'total_weight': 6.0, 'summary_thresholds': [1.0],
                     'max_mean_duration': [float(M.duration_mean(k).max()) for k in range(2)]}
    json.dumps(block)
