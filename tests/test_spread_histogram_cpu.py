"""CPU tests of the posterior predictive histograms (predictive.SpreadHistogram, ps_hist_*): the edge
table of bins= and its rejected inputs, the numpy reference of bin, quantile, bracket and exceedance on
hand-made counts, the quantile key tags, the result file with and without a histogram, and level
validation before any evaluation.  No device."""
import json
import types

import numpy as np
import pytest

from parasitoids_amd import predictive as PP

from hist_ref import exact_quantile, exceedance_from_counts, quantile_from_counts, weighted_counts


def test_default_edge_table_is_the_formula():
    e = PP.bin_edges()
    assert PP.DEFAULT_BINS == (1e-8, 1e6, 16)
    B = int(round(16 * np.log10(1e6 / 1e-8)))
    assert B == 224 and e.size == 225 and e.dtype == np.float64
    assert np.array_equal(e, 1e-8 * 10.0 ** (np.arange(B + 1) / 16))
    assert e[0] == 1e-8 and np.isclose(e[-1], 1e6, rtol=1e-12)
    assert np.allclose(e[1:] / e[:-1], 10 ** (1 / 16), rtol=1e-12)


@pytest.mark.parametrize('bins', [(1e-3, 1e3, 4), (0.5, 7.0, 3), (1e-8, 1e6, 1), (2.0, 2.5, 10)])
def test_edge_table_of_other_bins(bins):
    lo, hi, per = bins
    B = int(round(per * np.log10(hi / lo)))
    assert np.array_equal(PP.bin_edges(bins), lo * 10.0 ** (np.arange(B + 1) / per))


def test_explicit_edges_are_taken_as_given():
    src = [1e-6, 1e-3, 1.0, 3.0, 1e3]
    e = PP.bin_edges(edges=src)
    assert np.array_equal(e, src) and e.dtype == np.float64
    assert np.array_equal(PP.bin_edges((1, 2, 3), edges=src), src)     # edges= wins over bins=
    assert PP.bin_edges(edges=np.arange(1, 1025, dtype=float)).size == 1024


@pytest.mark.parametrize('bins', [(0.0, 1.0, 4), (-1e-8, 1.0, 4), (1.0, 1.0, 4), (1.0, 0.5, 4), (1e-8, 1e6, 0.5),
                                  (1e-8, 1e6, 0), (1e-8, 1e6, 80), (1e-8, np.inf, 4), (np.nan, 1.0, 4),
                                  (1.0, 1.01, 1), (1, 2)])
def test_rejected_bins(bins):
    with pytest.raises(ValueError):
        PP.bin_edges(bins)


@pytest.mark.parametrize('edges', [[1.0], [], [1.0, 1.0, 2.0], [2.0, 1.0], [0.0, 1.0], [-1.0, 1.0],
                                   [1.0, np.inf], [1.0, np.nan], np.arange(1, 1026, dtype=float)])
def test_rejected_edges(edges):
    with pytest.raises(ValueError):
        PP.bin_edges(edges=edges)


# ------------------------------------------------------------------ the numpy reference, by hand
EDGES = np.array([1.0, 2.0, 4.0, 8.0])          # B = 3: bins 0 [0, 1), 1 [1, 2), 2 [2, 4), 3 [4, 8), 4 [8, inf)


def test_bins_and_ties_at_edges():
    v = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 7.999, 8.0, 1e9])
    assert list(np.searchsorted(EDGES, v, side='right')) == [0, 0, 1, 1, 2, 3, 4, 4]
    c = weighted_counts([v], [3], EDGES)
    assert c.shape == (5, 8) and c.sum(0).tolist() == [3] * 8
    assert c[1, 2] == 3 and c[0, 2] == 0            # a value equal to an edge goes to the upper bin
    assert c[4, 6] == 3


def test_all_zero_cells():
    c = weighted_counts([np.zeros(3)] * 4, [1, 2, 1, 3], EDGES)
    assert c[0].tolist() == [7, 7, 7] and c[1:].sum() == 0
    for p in (0.05, 0.5, 1.0):
        b, val, lo, hi = quantile_from_counts(c, EDGES, p)
        assert b.tolist() == [0] * 3 and val.tolist() == [0.0] * 3
        assert lo.tolist() == [0.0] * 3 and hi.tolist() == [1.0] * 3
    assert exceedance_from_counts(c, 0).tolist() == [0.0] * 3


def test_quantile_in_bin_zero_mid_and_top():
    # one cell, weights: 6 at 0, 3 in [2, 4), 1 at 20 (top bin); W = 10
    fields = [np.array([0.0]), np.array([3.0]), np.array([20.0])]
    w = [6, 3, 1]
    c = weighted_counts(fields, w, EDGES)
    assert c[:, 0].tolist() == [6, 0, 3, 0, 1]
    b, val, lo, hi = quantile_from_counts(c, EDGES, 0.5)        # C_0 = 6 >= 5
    assert (b[0], val[0], lo[0], hi[0]) == (0, 0.0, 0.0, 1.0)
    b, val, lo, hi = quantile_from_counts(c, EDGES, 0.8)        # C_2 = 9 >= 8: f = (8 - 6) / 3
    assert (b[0], lo[0], hi[0]) == (2, 2.0, 4.0)
    assert val[0] == 2.0 * 2.0 ** (2.0 / 3.0)
    b, val, lo, hi = quantile_from_counts(c, EDGES, 1.0)        # p = 1: the top bin
    assert (b[0], val[0], lo[0], hi[0]) == (4, 8.0, 8.0, np.inf)
    b, val, lo, hi = quantile_from_counts(c, EDGES, 0.9)        # C_2 = 9 >= 9 exactly: f = 1, the upper edge
    assert (b[0], val[0]) == (2, 4.0)
    for p in (0.05, 0.5, 0.6, 0.61, 0.8, 0.9, 0.95, 1.0):
        q = exact_quantile(fields, w, p)
        _, _, lo, hi = quantile_from_counts(c, EDGES, p)
        assert lo[0] <= q[0] < hi[0], p


def test_ties_at_edges_in_quantiles_and_exceedance():
    fields = [np.array([1.0]), np.array([2.0]), np.array([2.0]), np.array([8.0])]
    w = [1, 1, 1, 1]
    c = weighted_counts(fields, w, EDGES)
    assert c[:, 0].tolist() == [0, 1, 2, 0, 1]
    assert exceedance_from_counts(c, 0)[0] == 1.0            # v >= 1: all
    assert exceedance_from_counts(c, 1)[0] == 0.75           # v >= 2: the tie counts
    assert exceedance_from_counts(c, 2)[0] == 0.25
    assert exceedance_from_counts(c, 3)[0] == 0.25           # v >= 8
    b, val, lo, hi = quantile_from_counts(c, EDGES, 0.5)
    assert exact_quantile(fields, w, 0.5)[0] == 2.0 and (lo[0], hi[0]) == (2.0, 4.0)
    b, val, lo, hi = quantile_from_counts(c, EDGES, 0.25)
    assert exact_quantile(fields, w, 0.25)[0] == 1.0 and (lo[0], hi[0]) == (1.0, 2.0) and val[0] == 2.0


def test_brackets_hold_the_exact_quantile_on_random_members():
    rng = np.random.default_rng(5)
    edges = PP.bin_edges((1e-4, 1e4, 4))
    fields = []
    for _ in range(9):
        f = 10 ** rng.uniform(-6, 5, size=200)
        f[rng.random(200) < 0.4] = 0.0
        f[:10] = edges[rng.integers(0, edges.size, 10)]         # values on the edges
        fields.append(f)
    w = rng.integers(1, 5, size=9)
    c = weighted_counts(fields, w, edges)
    for p in (0.05, 0.1, 0.5, 0.95, 1.0):
        q = exact_quantile(fields, w, p)
        b, val, lo, hi = quantile_from_counts(c, edges, p)
        assert np.all(lo <= q) and np.all(q < hi), p
        assert np.all(lo <= val) and np.all((val <= hi) | (b == edges.size)), p
    for k in range(edges.size):
        ref = (np.asarray(fields) >= edges[k]).astype(np.int64).T @ w / w.sum()
        assert np.array_equal(exceedance_from_counts(c, k), ref), k


def test_quantile_tags():
    assert [PP.quantile_tag(p) for p in (0.05, 0.5, 0.95, 0.025, 1.0, 0.001)] == \
        ['q5', 'q50', 'q95', 'q2p5', 'q100', 'q0p1']


def test_levels_are_checked():
    assert PP.check_levels((0.05, 0.5, 1)) == [0.05, 0.5, 1.0]
    for bad in ([0.0], [-0.1], [1.5], [0.5, float('nan')]):
        with pytest.raises(ValueError):
            PP.check_levels(bad)


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


class _Histogram():
    bins = (1e-8, 1e6, 16)

    def __init__(self):
        self.edges = PP.bin_edges(self.bins)
        self.asked = []

    def quantile(self, d, p):
        self.asked.append((d, p))
        m = np.zeros((5, 5))
        m[2, 2] = 100 * p + d
        return m


def _old_keys(days):
    keys = {'days'}
    for d in days:
        for suffix in ('', '_sd', '_pexc0'):
            keys |= {'%d%s_%s' % (100 + d, suffix, t) for t in ('data', 'ind', 'indptr')}
    return keys


def test_save_with_a_histogram_writes_the_quantile_maps(tmp_path):
    h = _Histogram()
    res = PP.PredictiveResult(_Summary([0, 2]), 3, 2, 0, 0.1, [], None, [], [0, 2], histogram=h,
                              quantiles=[0.05, 0.5, 0.95])
    npz, js = res.save(str(tmp_path / 'pp'))
    qkeys = {'%d_%s_%s' % (100 + d, q, t) for d in (0, 2) for q in ('q5', 'q50', 'q95') for t in ('data', 'ind', 'indptr')}
    with np.load(npz) as f:
        assert set(f.files) == _old_keys([0, 2]) | qkeys
        assert f['102_q50_data'].tolist() == [52.0] and f['102_q50_ind'].tolist() == [2]
    assert h.asked == [(0, 0.05), (0, 0.5), (0, 0.95), (2, 0.05), (2, 0.5), (2, 0.95)]
    meta = json.load(open(js))
    q = meta['predictive']['quantiles']
    assert q['levels'] == [0.05, 0.5, 0.95] and q['bins'] == [1e-8, 1e6, 16] and q['nedge'] == 225


def test_save_without_a_histogram_writes_todays_keys(tmp_path):
    res = PP.PredictiveResult(_Summary([0, 2]), 3, 2, 0, 0.1, [], None, [], [0, 2])
    assert res.histogram is None and res.quantiles is None
    npz, js = res.save(str(tmp_path / 'pp'))
    with np.load(npz) as f:
        assert set(f.files) == _old_keys([0, 2])
    meta = json.load(open(js))
    assert set(meta['predictive']) == {'thresholds', 'total_weight', 'members', 'rows', 'evaluations', 'failed',
                                       'chains'}


# ------------------------------------------------------------------ the driver
def _chain():
    from parasitoids_amd import mcmc
    names = [m[0] for m in mcmc.MODEL_BLOCK]
    t0 = np.array([m[2] for m in mcmc.MODEL_BLOCK])
    return np.array([t0, t0, t0 * 1.01]), names


@pytest.mark.parametrize('levels', [[0.5, 0.0], [-0.05], [1.01], [0.5, float('nan')]])
def test_levels_outside_the_unit_interval_raise_before_any_evaluation(levels):
    calls = []

    def evaluate(theta):
        calls.append(theta)
        return True
    with pytest.raises(ValueError):
        PP.posterior_predictive(None, _chain(), quantiles=levels, evaluate=evaluate)
    with pytest.raises(ValueError):
        PP.posterior_predictive(None, _chain(), quantiles=[0.5], bins=(1e-8, 1e6, 80), evaluate=evaluate)
    assert calls == []


def test_no_device_gives_no_histogram():
    res = PP.posterior_predictive(None, _chain(), quantiles=[0.05, 0.95], evaluate=lambda theta: True)
    assert res.summary is None and res.histogram is None and res.quantiles == [0.05, 0.95]
    res = PP.posterior_predictive(None, _chain(), evaluate=lambda theta: True)
    assert res.histogram is None and res.quantiles is None
