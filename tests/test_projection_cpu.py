"""CPU tests of the projections over time (predictive.emergence_weights / exposure_weights / check_weights,
ps_project_*): the emergence matrix against the literal loop of the reference's popdensity_to_emergence and
against Bayes_funcs._projection_matrix, its column sums, the exposure table, the numpy reference of the
arithmetic, and the refusals that need no device."""
import numpy as np
import pytest

from project_ref import project


def _literal_daily(collection_day, incubation_time, horizon=25):
    """the loop of the reference's Bayes_funcs.py:57-71 for a unit population at one cell:
    emerg[day - start, day post collection]"""
    start_day = max(collection_day - horizon, 0)
    emerg_proj = np.zeros((collection_day - start_day, horizon))
    for day in range(start_day, collection_day):
        max_post_col = day + horizon - collection_day
        min_post_col = max(0, max_post_col + 1 - incubation_time.size)
        span_len = max_post_col - min_post_col + 1
        e_distrib = 1.0 * incubation_time
        emerg_proj[day - start_day, min_post_col:max_post_col + 1] += e_distrib[-span_len:]
    return start_day, emerg_proj


@pytest.mark.parametrize('cday', [3, 6, 20, 30])
def test_daily_emergence_weights_are_the_reference_loop(cday):
    from parasitoids_amd import Bayes_funcs as BF
    from parasitoids_amd.predictive import emergence_weights
    start, emerg = _literal_daily(cday, BF.incubation_time)
    in_days = list(range(start, cday))
    W = emergence_weights(cday, in_days)
    assert W.shape == (25, len(in_days)) and W.dtype == np.float64
    assert np.array_equal(W, emerg.T)
    # a wider list of input days: the same weights in the oviposition days' columns, zeros elsewhere
    wide = list(range(0, cday + 2))
    Ww = emergence_weights(cday, wide)
    assert np.array_equal(Ww[:, start:cday], W) and not Ww[:, cday:].any() and not Ww[:, :start].any()


@pytest.mark.parametrize('cday,obs', [(3, [3, 5, 9, 20, 26]), (6, [8, 14, 22, 30]), (20, [20, 21, 30, 44]),
                                       (30, [33, 40, 41, 54])])
def test_binned_emergence_weights_are_the_projection_matrix_transposed(cday, obs):
    from parasitoids_amd import Bayes_funcs as BF
    from parasitoids_amd.predictive import emergence_weights
    start = max(cday - 25, 0)
    W = emergence_weights(cday, range(start, cday), obs)
    assert np.array_equal(W, BF._projection_matrix(start, cday, np.array(obs)).T)
    # the bins partition the daily matrix up to the last observation day
    daily = emergence_weights(cday, range(start, cday))
    np.testing.assert_allclose(W.sum(0), daily[:obs[-1] - cday + 1].sum(0), rtol=0, atol=1e-15)


@pytest.mark.parametrize('cday', [3, 6, 20, 30])
def test_daily_columns_sum_to_the_share_emerging_after_collection(cday):
    from parasitoids_amd import Bayes_funcs as BF
    from parasitoids_amd.predictive import emergence_weights
    start = max(cday - 25, 0)
    W = emergence_weights(cday, range(start, cday))
    inc = BF.incubation_time                       # incubation of 19 + k days has probability inc[k]
    for n, day in enumerate(range(start, cday)):
        share = sum(p for k, p in enumerate(inc) if day + 19 + k >= cday)
        assert abs(W[:, n].sum() - share) <= 1e-15, (day, W[:, n].sum(), share)
        if day >= cday - 19:
            assert abs(W[:, n].sum() - 1.0) <= 1e-15


def test_exposure_weights_are_the_stated_table():
    from parasitoids_amd.predictive import exposure_weights
    W = exposure_weights([0, 1, 2, 3, 4, 5], [0, 2, 5])
    assert W.dtype == np.float64
    assert np.array_equal(W, [[1, 0, 0, 0, 0, 0], [1, 1, 1, 0, 0, 0], [1, 1, 1, 1, 1, 1]])
    W = exposure_weights([1, 3, 7], [0, 3, 6, 7])
    assert np.array_equal(W, [[0, 0, 0], [1, 1, 0], [1, 1, 0], [1, 1, 1]])


def test_numpy_reference_rounds_product_and_sum_separately():
    rng = np.random.default_rng(0)
    f = rng.random((4, 5, 3)) * 1e3
    W = np.array([[0.05, 0.0, 0.3, 0.2], [0.0, 0.0, 0.0, 1.0], [1.0, 1.0, 1.0, 1.0]])
    Y = project(f, W)
    assert np.array_equal(Y[0], (0.0 + 0.05 * f[0] + 0.3 * f[2]) + 0.2 * f[3])
    assert np.array_equal(Y[1], f[3])
    assert np.array_equal(Y[2], ((f[0] + f[1]) + f[2]) + f[3])


def test_refusals_before_any_device_work():
    from parasitoids_amd.predictive import (check_in_days, check_weights, emergence_plan, emergence_weights,
                                            exposure_plan)
    # a missing oviposition day that carries weight is never dropped silently
    with pytest.raises(ValueError, match='oviposition day 2'):
        emergence_weights(6, [0, 1, 3, 4, 5])
    with pytest.raises(ValueError, match='oviposition day'):
        emergence_weights(30, range(6, 30))          # day 5 = 30 - 25 emerges on the collection day
    with pytest.raises(ValueError):
        emergence_weights(6, range(6), [5, 8])       # an observation before the collection
    ok = np.array([[1.0, 0.0], [0.5, 0.5]])
    assert np.array_equal(check_weights(ok, 2), ok)
    for bad in (-1e-300, -1.0, np.nan, np.inf):
        W = ok.copy()
        W[1, 0] = bad
        with pytest.raises(ValueError, match='finite and >= 0'):
            check_weights(W, 2)
    with pytest.raises(ValueError, match='no non-zero weight'):
        check_weights([[1.0, 0.0], [0.0, 0.0]], 2)
    with pytest.raises(ValueError, match='inputs'):
        check_weights(np.ones((2, 33)))
    with pytest.raises(ValueError, match='outputs'):
        check_weights(np.ones((33, 2)))
    with pytest.raises(ValueError):
        check_weights(np.ones((2, 3)), 2)            # columns against the input days
    with pytest.raises(ValueError):
        check_weights(np.ones(3))
    with pytest.raises(ValueError):
        check_in_days(range(33))
    with pytest.raises(ValueError):
        check_in_days([0, 2, 2])
    assert check_weights(np.ones((32, 32))).shape == (32, 32) and check_in_days(range(32)) == list(range(32))
    # the arguments of posterior_predictive
    W, in_days, labels = emergence_plan(dict(collection_day=6), 6)
    assert W.shape == (25, 6) and in_days == list(range(6)) and labels == list(range(6, 31))
    W, in_days, labels = emergence_plan(dict(collection_day=6, obs_days=[8, 30]), 6)
    assert W.shape == (2, 6) and labels == [8, 30]
    with pytest.raises(ValueError):
        emergence_plan(dict(collection_day=7), 6)    # the model does not reach day 6
    with pytest.raises(ValueError):
        emergence_plan(dict(day=6), 6)
    with pytest.raises(ValueError):
        emergence_plan(dict(collection_day=0), 6)
    W, in_days, labels = exposure_plan([2, 5], 6)
    assert W.shape == (2, 6) and in_days == list(range(6)) and labels == [2, 5]
    for bad in ([], [5, 2], [-1, 2], [2, 6], [40]):
        with pytest.raises(ValueError):
            exposure_plan(bad, 6)


def test_posterior_predictive_refuses_bad_projection_arguments_before_evaluating():
    from parasitoids_amd.predictive import posterior_predictive
    calls = []
    trace = np.zeros((3, 1))

    def evaluate(theta):
        calls.append(theta)
        return None
    for kw in (dict(emergence=dict(collection_day=0)), dict(emergence=[6]), dict(exposure=[3, 1]),
               dict(exposure=[32])):
        with pytest.raises(ValueError, match='emergence must be|collection day|exposure days|input days'):
            posterior_predictive(None, (trace, ['x']), evaluate=evaluate, **kw)
    assert not calls
