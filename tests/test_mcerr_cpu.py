"""CPU tests of the Monte Carlo error of the posterior maps: the numpy replay (mcerr_ref) of ps_mcerr_* against
closed-form two-pass batch means, its exact integer counts, the library's split of a weight, merge and finish,
predictive.mc_batch_plan and the split of a run at a chain's half, the refusals of posterior_predictive before any
evaluation, and a sanity check of the definitions on AR(1) series whose effective sample size is known."""
import numpy as np
import pytest

import mcerr_ref
from parasitoids_amd.predictive import (MonteCarloError, check_mc_thresholds, mc_batch_plan, mc_error_plan, mc_split,
                                        posterior_predictive)


def _fields(rng, members, shape=(7, 9)):
    """random sparse-ish non-negative fields: zeros (constant cells), repeated members, values around the thresholds"""
    f = rng.gamma(0.6, 8.0, size=(members,) + shape)
    f[:, :2] = 0.0
    f[:, 2, :3] = 5.0
    f[3] = f[2]
    return f


def _rows(fields, weights):
    return np.repeat(fields, weights, axis=0)


def test_the_split_of_a_weight():
    assert mcerr_ref.pieces(0, 3, 1) == [1] and mcerr_ref.pieces(2, 3, 1) == [1]
    assert mcerr_ref.pieces(2, 3, 4) == [1, 3] and mcerr_ref.pieces(1, 3, 9) == [2, 3, 3, 1]
    assert mcerr_ref.pieces(0, 1, 3) == [1, 1, 1] and mcerr_ref.pieces(0, 5, 4) == [4]


def test_the_replay_matches_two_pass_batch_means():
    rng = np.random.default_rng(3)
    weights = [1, 3, 1, 2, 1, 4, 2, 1, 3, 2, 1, 3, 2]        # 26 rows: 8 batches of 3 and 2 rows discarded
    f = _fields(rng, len(weights))
    thr = [1.0, 10.0]
    st = mcerr_ref.new_state(f.shape[1:], thr, 3)
    for v, w in zip(f, weights):
        mcerr_ref.add(st, v, w)
    assert (st['B'], st['open'], st['discarded'], st['members']) == (8, 2, 0, 13)
    assert st['bmean'].any() and st['bcnt'].any()
    mcerr_ref.finish(st)
    assert (st['B'], st['open'], st['discarded']) == (8, 0, 2) and not st['bmean'].any() and not st['bcnt'].any()
    ref = mcerr_ref.two_pass(_rows(f, weights), 3, thr)
    assert ref['B'] == 8 and ref['n'] == 24 == mcerr_ref.used(st)
    scale = f.max()
    kw = dict(rtol=1e-12, atol=1e-14 * scale)
    np.testing.assert_allclose(st['gmean'], ref['mean'], **kw)
    np.testing.assert_allclose(mcerr_ref.mcse(st), ref['mcse'], rtol=1e-10, atol=1e-14 * scale)
    np.testing.assert_allclose(mcerr_ref.variance(st), ref['variance'], rtol=1e-11, atol=1e-14 * scale ** 2)
    np.testing.assert_allclose(mcerr_ref.ess(st), ref['ess'], rtol=1e-9)
    # constant cells: nothing varies, and the ESS is 0 by definition, not a division by zero
    assert not st['gM2'][:2].any() and not mcerr_ref.ess(st)[:2].any() and not mcerr_ref.mcse(st)[2, :3].any()
    assert (mcerr_ref.ess(st)[3:] > 0).all()
    for k in range(2):
        s1, s2, pm = ref['thr'][k]
        assert np.array_equal(st['s1'][k].astype(np.int64), s1) and np.array_equal(st['s2'][k].astype(np.int64), s2)
        num = mcerr_ref.count_variance_numerator(st, k)
        assert (num >= 0).all() and (num > 0).any()
        np.testing.assert_allclose(mcerr_ref.prob_mcse(st, k), pm, rtol=1e-12, atol=1e-15)
    # the caller's own split and unit adds: the counts are the same integers
    unit = mcerr_ref.new_state(f.shape[1:], thr, 3)
    own = mcerr_ref.new_state(f.shape[1:], thr, 3)
    for v, w in zip(f, weights):
        for p in mcerr_ref.pieces(own['open'], 3, w):
            mcerr_ref.add_piece(own, v, p)
        for _ in range(w):
            mcerr_ref.add(unit, v, 1)
    for other in (mcerr_ref.finish(unit), mcerr_ref.finish(own)):
        assert np.array_equal(other['s1'], st['s1']) and np.array_equal(other['s2'], st['s2']) and other['B'] == 8
    assert np.array_equal(own['gmean'], st['gmean']) and np.array_equal(own['gM2'], st['gM2'])
    np.testing.assert_allclose(unit['gmean'], st['gmean'], rtol=1e-13)


def test_counts_stay_exact_near_the_top_of_the_range():
    """b close to 2^32: s2 = c^2 needs all 64 bits, and B s2 - s1^2 is formed without rounding"""
    b = 2 ** 31 - 1
    st = mcerr_ref.new_state((2,), [1.0], b)
    mcerr_ref.add(st, np.array([2.0, 0.0]), b)
    mcerr_ref.add(st, np.array([2.0, 2.0]), b - 1)
    mcerr_ref.add(st, np.array([0.0, 2.0]), 1)
    assert st['B'] == 2 and st['open'] == 0
    assert [int(x) for x in st['s1'][0]] == [2 * b - 1, b] and [int(x) for x in st['s2'][0]] == [b * b + (b - 1) ** 2, b * b]
    assert list(mcerr_ref.count_variance_numerator(st, 0)) == [1, b * b]


def test_merge_pools_the_closed_batches():
    rng = np.random.default_rng(5)
    f = _fields(rng, 12)
    weights = [2] * 12
    whole = mcerr_ref.new_state(f.shape[1:], [1.0], 4)
    lo, hi = mcerr_ref.new_state(f.shape[1:], [1.0], 4), mcerr_ref.new_state(f.shape[1:], [1.0], 4)
    for i, (v, w) in enumerate(zip(f, weights)):
        mcerr_ref.add(whole, v, w)
        mcerr_ref.add(lo if i < 4 else hi, v, w)
    empty = mcerr_ref.merge(mcerr_ref.new_state(f.shape[1:], [1.0], 4), lo)
    assert all(np.array_equal(empty[k], lo[k]) for k in ('gmean', 'gM2', 'wM2', 's1', 's2')) and empty['B'] == 2
    mcerr_ref.merge(lo, hi)
    assert lo['B'] == whole['B'] == 6 and lo['members'] == 12
    assert np.array_equal(lo['s1'], whole['s1']) and np.array_equal(lo['s2'], whole['s2'])
    np.testing.assert_allclose(lo['gmean'], whole['gmean'], rtol=1e-12, atol=1e-14 * f.max())
    np.testing.assert_allclose(lo['gM2'], whole['gM2'], rtol=1e-11, atol=1e-14 * f.max() ** 2)
    np.testing.assert_allclose(lo['wM2'], whole['wM2'], rtol=1e-12)


def test_mc_batch_plan():
    assert mc_batch_plan([300], 20) == (15, [(150, 300)])
    assert mc_batch_plan([301, 97, 40], 4) == (10, [(150, 301), (48, 97), (20, 40)])      # uneven chains share one b
    assert mc_batch_plan([4], 4) == (1, [(2, 4)])
    for bad in (3, 5, 2, 0, -4, 4.5):
        with pytest.raises(ValueError, match='even integer >= 4'):
            mc_batch_plan([100], bad)
    with pytest.raises(ValueError, match='shorter than 20 batches'):
        mc_batch_plan([300, 19], 20)
    with pytest.raises(ValueError, match='no chains'):
        mc_batch_plan([], 4)
    # a run against the half boundary: before it, straddling it, from it on
    assert mc_split(0, 3, 5) == (3, 0) and mc_split(3, 2, 5) == (2, 0) and mc_split(3, 4, 5) == (2, 2)
    assert mc_split(5, 2, 5) == (0, 2) and mc_split(7, 1, 5) == (0, 1) and mc_split(0, 10, 5) == (5, 5)
    assert mc_error_plan(True) == 20 and mc_error_plan({}) == 20 and mc_error_plan(dict(batches=6)) == 6
    for bad in (dict(batches=5), dict(batch=4), 20, 'yes'):
        with pytest.raises(ValueError):
            mc_error_plan(bad)
    assert check_mc_thresholds((1, 10)) == [1.0, 10.0] and check_mc_thresholds(()) == []
    for bad in ([2.0, 1.0], [1.0, 1.0], [np.nan], [np.inf], [1, 2, 3, 4, 5]):
        with pytest.raises(ValueError):
            check_mc_thresholds(bad)
    assert callable(MonteCarloError.for_projection)


def test_posterior_predictive_refuses_before_any_evaluation():
    from parasitoids_amd import mcmc
    names = [m[0] for m in mcmc.MODEL_BLOCK]
    trace = np.tile(np.array([m[2] for m in mcmc.MODEL_BLOCK], dtype=np.float64), (9, 1))
    trace[4:, names.index('mu_r')] += 0.1
    calls = []

    class Untouchable():
        def __getattr__(self, name):
            calls.append(name)
            raise AssertionError('the model was touched: ' + name)

    def evaluate(theta):
        calls.append('evaluate')
    with pytest.raises(ValueError, match='not with evaluate='):
        posterior_predictive(None, (trace, names), evaluate=evaluate, mc_error=True)
    with pytest.raises(ValueError, match='even integer >= 4'):
        posterior_predictive(Untouchable(), (trace, names), mc_error=dict(batches=5))
    with pytest.raises(ValueError, match='must be True or dict'):
        posterior_predictive(Untouchable(), (trace, names), mc_error=dict(batch=4))
    with pytest.raises(ValueError, match='9 rows is shorter than 20 batches'):
        posterior_predictive(Untouchable(), (trace, names), mc_error=True)
    with pytest.raises(ValueError, match='7 rows is shorter than 8 batches'):
        posterior_predictive(Untouchable(), (trace, names), burn=2, mc_error=dict(batches=8))
    with pytest.raises(ValueError, match='strictly increasing'):
        posterior_predictive(Untouchable(), (trace, names), thresholds=(10.0, 1.0), mc_error=dict(batches=4))
    assert calls == []


def test_the_definitions_on_ar1_series():
    """AR(1) with rho = 0.5: ESS / n -> (1 - rho) / (1 + rho) = 1/3, and chains from one distribution have a
    split R-hat of 1.  2 chains x 2000 rows over 256 independent cells, b = 25, fed to the replay in halves."""
    rho, nrow, ncell, b = 0.5, 2000, 256, 25
    rng = np.random.default_rng(7)
    seqs = []
    for _chain in range(2):
        e = rng.standard_normal((nrow, ncell))
        x = np.empty((nrow, ncell))
        x[0] = e[0] / np.sqrt(1.0 - rho * rho)
        for t in range(1, nrow):
            x[t] = rho * x[t - 1] + e[t]
        for half in (x[:nrow // 2], x[nrow // 2:]):
            st = mcerr_ref.new_state((ncell,), [], b)
            for row in half:
                mcerr_ref.add(st, row, 1)
            seqs.append(mcerr_ref.finish(st))
    assert [s['B'] for s in seqs] == [40] * 4
    r = mcerr_ref.rhat([mcerr_ref.state_planes(s) for s in seqs], b)
    pooled = seqs[0]
    for s in seqs[1:]:
        mcerr_ref.merge(pooled, s)
    assert pooled['B'] == 160 and mcerr_ref.used(pooled) == 2 * nrow
    ratio = np.median(mcerr_ref.ess(pooled)) / mcerr_ref.used(pooled)
    want = (1.0 - rho) / (1.0 + rho)
    print('median ESS / n %.4f against %.4f, median split R-hat %.5f' % (ratio, want, np.median(r)))
    assert abs(ratio - want) <= 0.2 * want
    assert abs(np.median(r) - 1.0) <= 0.01
