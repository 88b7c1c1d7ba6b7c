"""CPU tests of the weather ensembles: the moving-block bootstrap of the wind record (predictive.wind_sequences), the
checks of wind= (check_wind, _check_request) and the arithmetic of the variance split on its numpy replay
(weather_ref.NestedReplay, the statements of ps_nested_*) against the closed forms, on numbers chosen so that every
operation is exact."""
import types

import numpy as np
import pytest

from weather_ref import NestedReplay, closed_form

from parasitoids_amd import predictive as PR


# ---------------------------------------------------------------- the plan
def _successor(pool, day):
    return pool[(pool.index(day) + 1) % len(pool)]


@pytest.mark.parametrize('pool, ndays, draws, block', [
    (list(range(1, 19)), 18, 8, 3), (list(range(1, 31)), 30, 5, 4), ([3, 4, 7, 9, 20], 6, 4, 1),
    ([3, 4, 7, 9, 20], 7, 3, 7), ([3, 4, 7, 9, 20], 7, 3, 50), ([5, 11], 9, 6, 3), ([5, 11], 1, 2, 3)])
def test_wind_sequences_are_circular_blocks_of_the_pool(pool, ndays, draws, block):
    seqs = PR.wind_sequences(pool, ndays, draws, block=block, seed=4)
    assert seqs.shape == (draws, ndays) and np.issubdtype(seqs.dtype, np.integer)
    assert set(seqs.ravel().tolist()) <= set(pool)
    assert np.array_equal(seqs, PR.wind_sequences(pool, ndays, draws, block=block, seed=4))
    for row in seqs.tolist():
        for i in range(1, ndays):
            if i % block:                  # inside a block: the circular successor of the entry before
                assert row[i] == _successor(pool, row[i - 1]), (row, i)
    if ndays > 1 and draws * ndays >= 12:
        other = PR.wind_sequences(pool, ndays, draws, block=block, seed=5)
        assert other.shape == seqs.shape and not np.array_equal(other, seqs)


def test_wind_sequences_take_their_starts_from_pcg64():
    pool = [2, 3, 5, 8, 13, 21]
    seqs = PR.wind_sequences(pool, 7, 4, block=3, seed=11)
    starts = np.random.Generator(np.random.PCG64(11)).integers(0, len(pool), size=(4, 3))
    assert np.array_equal(seqs[:, ::3], np.asarray(pool)[starts])


@pytest.mark.parametrize('pool, ndays, draws, block, seed', [
    ([4], 3, 2, 3, 0), ([], 3, 2, 3, 0), ([4, 4, 5], 3, 2, 3, 0), ([5, 4], 3, 2, 3, 0), ([1, 2], 0, 2, 3, 0),
    ([1, 2], 3, 0, 3, 0), ([1, 2], 3, 2, 0, 0), ([1, 2], 3, 2, 3, -1), ([1, 2], 3.0, 2, 3, 0), ([1, 2], 3, True, 3, 0)])
def test_wind_sequences_refuse(pool, ndays, draws, block, seed):
    with pytest.raises(ValueError, match='wind'):
        PR.wind_sequences(pool, ndays, draws, block=block, seed=seed)


def _model(ndays=6, record=range(1, 31)):
    return types.SimpleNamespace(wind_data={d: None for d in record}, days=list(record)[:ndays], rad_dist=10000.0,
                                 rad_res=64)


def test_check_wind_defaults_and_given_sequences():
    pm = _model()
    plan = PR.check_wind({}, pm)
    assert plan['draws'] == 8 and plan['block'] == 3 and plan['seed'] == 0 and plan['share'] and plan['pool_kernels']
    assert plan['pool'] == list(range(1, 31)) and plan['sequences'].shape == (8, 6)
    assert np.array_equal(plan['sequences'], PR.wind_sequences(range(1, 31), 6, 8, 3, 0))
    assert plan['used'] == sorted(set(plan['sequences'].ravel().tolist()))
    plan = PR.check_wind(dict(draws=3, block=2, seed=9, pool=[9, 4, 4, 7], share=False, pool_kernels=False), pm)
    assert plan['pool'] == [4, 7, 9] and plan['sequences'].shape == (3, 6) and not plan['share']
    assert not plan['pool_kernels'] and set(plan['used']) <= {4, 7, 9}
    given = [[1, 2, 3, 4, 5, 6], [6, 5, 4, 3, 2, 1], [30, 30, 1, 1, 2, 2]]
    plan = PR.check_wind(dict(sequences=given, draws=50), pm)
    assert plan['sequences'].tolist() == given and plan['draws'] == 3 and plan['used'] == [1, 2, 3, 4, 5, 6, 30]
    assert PR.check_wind(dict(sequences=given[:1], share=False), pm)['sequences'].tolist() == given[:1]
    assert PR.check_wind(dict(draws=1, share=False), pm)['sequences'].shape == (1, 6)


@pytest.mark.parametrize('arg', [
    [1, 2], 'yes', dict(draw=3), dict(draws=0), dict(draws=2.0), dict(draws=True), dict(block=0), dict(seed=-1),
    dict(share=1), dict(pool_kernels='no'), dict(pool=[1]), dict(pool=[1, 1]), dict(pool=[1, 99]), dict(pool=[1, 2.5]),
    dict(pool=7), dict(draws=1), dict(sequences=[[1, 2, 3, 4, 5, 6]]), dict(sequences=[]),
    dict(sequences=[[1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5]]), dict(sequences=[[1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 77]]),
    dict(sequences=[[1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 'x']]), dict(sequences=5)])
def test_check_wind_refuses(arg):
    with pytest.raises(ValueError, match='wind'):
        PR.check_wind(arg, _model())


FINDING = (0.0, 0.0, 1, 'none', 0.1)
CHAIN = (np.zeros((2, 15)), ['x'])             # never loaded: the refusals come first


@pytest.mark.parametrize('name, extra', [
    ('evaluate', dict(evaluate=lambda theta: None)), ('locinfo', dict(locinfo=object())),
    ('reweight', dict(reweight={'a': dict(probes=[FINDING])})), ('origin', dict(origin=[FINDING])),
    ('mc_error', dict(mc_error=True)), ('representative', dict(representative=True, excursion=[1.0])),
    ('sensitivity', dict(sensitivity=True)), ('dependence', dict(dependence=True))])
def test_the_request_refuses_wind_with(name, extra):
    with pytest.raises(ValueError, match='wind= does not go with %s=' % name):
        PR.posterior_predictive(_model(), CHAIN, wind=dict(draws=2), **extra)


@pytest.mark.parametrize('name, extra', [
    ('sites', dict(sites=dict(sites=[(0.0, 0.0, 1.0), (100.0, 0.0, 1.0, 2)]))),
    ('compare', dict(sites=dict(sites=[(0.0, 0.0, 1.0)]), compare=dict(sites=[(0.0, 0.0, 0.5), (0.0, 0.0, 0.5, 1)]))),
    ('ranking', dict(sites=dict(sites=[(0.0, 0.0, 1.0)]),
                     ranking=[dict(sites=[(100.0, 0.0, 1.0)]), dict(sites=[(0.0, 100.0, 0.5), (0.0, 100.0, 0.5, 3)])]))])
def test_the_request_refuses_wind_with_a_later_release(name, extra):
    with pytest.raises(ValueError, match='wind= does not go with a plan of %s= that releases after day 0' % name):
        PR.posterior_predictive(_model(), CHAIN, thresholds=(1.0,), wind=dict(draws=2), **extra)


def test_the_request_checks_the_wind_argument_before_any_chain_is_loaded():
    with pytest.raises(ValueError, match='wind: draws'):
        PR.posterior_predictive(_model(), CHAIN, wind=dict(draws=0))
    with pytest.raises(ValueError, match='at least 2 sequences'):
        PR.posterior_predictive(_model(), CHAIN, wind=dict(draws=1))
    with pytest.raises(ValueError, match='wind= needs a PopModel'):
        PR.posterior_predictive(None, CHAIN, wind=dict(draws=2))


def test_the_driver_tables_hold_the_weather_share():
    for kind in ('days', 'projection', 'sites'):
        order = PR.FEED_ORDER[kind]
        assert order.index('weather') > order.index('summary')
    for kind in ('compare', 'ranking'):
        assert 'weather' not in PR.FEED_ORDER[kind]
    assert 'weather' in PR.ACCUMULATORS and PR.BUILD['weather'] is PR._build_weather and 'weather' in PR.FEED
    fs = PR._FieldSet().fed_from('days', object(), owns=False)       # the source is no model: building would raise
    for q in (types.SimpleNamespace(), types.SimpleNamespace(wind_plan=None),
              types.SimpleNamespace(wind_plan=dict(share=False))):
        assert PR._build_weather(fs, q) is None


# ---------------------------------------------------------------- the arithmetic
def _planes(seed=3, shape=(5, 7)):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 40, size=(3,) + shape).astype(np.float64), rng.integers(0, 6, size=shape).astype(np.float64)


def _feed(groups, weights, shape):
    r = NestedReplay(shape)
    for g, w in zip(groups, weights):
        for v in g:
            r.add(v)
        r.close(w)
    return r


def test_the_replay_equals_the_closed_form_exactly_on_integer_planes():
    a, c = _planes()
    groups = [np.array([a[g] - c, a[g] + c]) for g in range(3)]      # v = a_g + e_b, e = (-c, +c)
    weights = [1, 1, 2]
    r = _feed(groups, weights, a.shape[1:])
    assert (r.G, r.W, r.members, r.k, r.wk) == (3, 4.0, 6, 0, 2.0)
    got, want = r.finalize(), closed_form(groups, weights)
    assert np.array_equal(want['vw'], 2.0 * c * c)                   # the sample variance of (-c, +c)
    for name in ('vw', 'vm', 'vp', 'share'):
        assert np.array_equal(got[name], want[name]), name
    assert np.array_equal(r.omean, want['mean'])
    assert (want['vp'] > 0).any() and (want['vp'] == 0).any() and ((got['share'] > 0) & (got['share'] < 1)).any()
    assert not r.imean.any() and not r.iM2.any()


def test_identical_draws_leave_no_weather():
    a, _c = _planes(5)
    r = _feed([np.array([a[g], a[g], a[g]]) for g in range(3)], [1, 3, 2], a.shape[1:])
    out = r.finalize()
    assert not out['vw'].any() and not out['share'].any() and not np.signbit(out['share']).any()
    assert np.array_equal(out['vp'], out['vm']) and out['vp'].max() > 0


def test_identical_groups_leave_no_parameter_variance():
    a, c = _planes(7)
    g = np.array([a[0] - 3 * c, a[0], a[0] + 3 * c])
    r = _feed([g, g, g], [1, 3, 2], a.shape[1:])
    out = r.finalize()
    assert not r.oM2.any() and not out['vp'].any()
    assert np.array_equal(out['share'], (c > 0).astype(np.float64)) and (c == 0).any() and (c > 0).any()
    assert np.array_equal(out['vw'], 9.0 * c * c)


def test_unequal_group_sizes_use_kinv():
    a, c = _planes(9)
    groups = [np.array([a[0] - c, a[0] + c]), np.array([a[1] - 3 * c, a[1], a[1], a[1] + 3 * c])]
    r = _feed(groups, [1, 1], a.shape[1:])
    assert r.wk == 0.75 and r.W == 2.0
    got, want = r.finalize(), closed_form(groups, [1, 1])
    assert np.array_equal(want['vw'], (2.0 * c * c + 6.0 * c * c) / 2.0)
    for name in ('vw', 'vm', 'vp', 'share'):
        assert np.array_equal(got[name], want[name]), name
    assert np.array_equal(got['vp'], np.maximum(got['vm'] - got['vw'] * 0.375, 0.0))
    wrong = np.maximum(got['vm'] - got['vw'] * 0.5, 0.0)             # every group taken for two draws
    assert not np.array_equal(got['vp'], wrong)


def test_merging_two_halves_pools_the_groups():
    a, c = _planes(11)
    groups = [np.array([a[g] - (g + 1) * c, a[g] + (g + 1) * c]) for g in range(3)] + [np.array([a[0], a[1], a[2]])]
    weights = [1, 3, 2, 2]
    whole = _feed(groups, weights, a.shape[1:])
    left, right = _feed(groups[:2], weights[:2], a.shape[1:]), _feed(groups[2:], weights[2:], a.shape[1:])
    empty = NestedReplay(a.shape[1:])
    empty.merge(left)
    assert np.array_equal(empty.omean, left.omean) and empty.G == 2
    left.merge(right)
    assert (left.G, left.W, left.members, left.wk) == (whole.G, whole.W, whole.members, whole.wk)
    got, want = left.finalize(), closed_form(groups, weights)
    np.testing.assert_allclose(left.omean, want['mean'], rtol=1e-14)
    for name in ('vw', 'vm', 'vp', 'share'):
        np.testing.assert_allclose(got[name], want[name], rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(got[name], whole.finalize()[name], rtol=1e-13, atol=1e-13)
