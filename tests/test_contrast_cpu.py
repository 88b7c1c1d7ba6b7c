"""CPU tests of the paired contrast of two plans (predictive.PlanContrast): the numpy reference (contrast_ref)
against three identities that hold bit for bit -- swapping the sides, halving one side, equal sides --
coverage_difference against cases worked out by hand, and every refusal that needs no device."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import contrast_ref
import sens_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = [1, 3, 1, 2, 1, 4]
THR = [0.5, 4.0]


def _sparse_fields(seed, shape=(9, 9)):
    """one random sparse field per weight: mostly zeros, the rest spread over four decades"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in WEIGHTS:
        f = 10.0 ** rng.uniform(-2, 2, size=shape)
        f[rng.random(shape) < 0.6] = 0.0
        out.append(f)
    return out


def _fill(A, B):
    st = contrast_ref.new_state(A[0].shape, THR)
    for a, b, w in zip(A, B, WEIGHTS):
        contrast_ref.add(st, a, b, w)
    return st


def test_swapping_the_sides_negates_the_mean_and_swaps_the_counts():
    A, B = _sparse_fields(1), _sparse_fields(2)
    ab, ba = _fill(A, B), _fill(B, A)
    assert ab['W'] == ba['W'] == sum(WEIGHTS) and ab['weights'] == WEIGHTS
    assert ab['pos'].max() > 0 and ab['neg'].max() > 0 and ab['gain'].max() > 0 and ab['loss'].max() > 0
    assert np.array_equal(ba['mean'], -ab['mean']) and np.abs(ab['mean']).max() > 0
    assert np.array_equal(ba['M2'], ab['M2']) and ab['M2'].max() > 0
    assert np.array_equal(ba['pos'], ab['neg']) and np.array_equal(ba['neg'], ab['pos'])
    assert np.array_equal(ba['gain'], ab['loss']) and np.array_equal(ba['loss'], ab['gain'])
    assert ba['cells_a'] == ab['cells_b'] and ba['cells_b'] == ab['cells_a'] and ab['cells_a'] != ab['cells_b']
    # against the plain definitions
    d = np.array(A) - np.array(B)
    mean, var = contrast_ref.two_pass(d, WEIGHTS)
    np.testing.assert_allclose(ab['mean'], mean, rtol=1e-12, atol=1e-15 * np.abs(d).max())
    np.testing.assert_allclose(ab['M2'] / ab['W'], var, rtol=1e-12, atol=1e-15 * np.abs(d).max() ** 2)
    w = np.array(WEIGHTS).reshape(-1, 1, 1)
    assert np.array_equal(ab['pos'], (w * (d > 0)).sum(0)) and np.array_equal(ab['neg'], (w * (d < 0)).sum(0))
    for k, t in enumerate(THR):
        assert np.array_equal(ab['gain'][k], (w * ((np.array(A) >= t) & (np.array(B) < t))).sum(0))
        assert [r[k] for r in ab['cells_b']] == [int((b >= t).sum()) for b in B]
    assert len(contrast_ref.planes(ab)) == 6 and np.array_equal(contrast_ref.planes(ab)[3], ab['loss'][0])


def test_half_of_a_plan_against_the_plain_accumulation():
    A = _sparse_fields(3)
    st = _fill(A, [0.5 * a for a in A])
    west = sens_ref.new_state(A[0].shape, 0)
    for a, w in zip(A, WEIGHTS):
        sens_ref.add(west, a, [], w)
    assert np.array_equal(st['mean'], 0.5 * west['mean']) and west['mean'].max() > 0
    assert np.array_equal(st['M2'], 0.25 * west['M2']) and west['M2'].max() > 0
    assert not st['neg'].any() and np.array_equal(st['pos'], sum(w * (a > 0) for a, w in zip(A, WEIGHTS)))
    assert not st['loss'].any() and st['gain'].max() > 0


def test_equal_plans_leave_everything_zero():
    A = _sparse_fields(4)
    st = _fill(A, [a.copy() for a in A])
    for key in ('mean', 'M2', 'pos', 'neg', 'gain', 'loss'):
        assert not st[key].any(), key
    assert st['cells_a'] == st['cells_b'] and max(max(r) for r in st['cells_a']) > 0 and st['W'] == sum(WEIGHTS)


def test_coverage_difference_by_hand():
    from parasitoids_amd.predictive import coverage_difference
    # four members, two outputs; the differences: output 0 -> [2, -3, 0, -3], output 1 -> [1, 1, 1, 1]
    a = np.array([[5, 4], [1, 3], [2, 2], [0, 9]])
    b = np.array([[3, 3], [4, 2], [2, 1], [3, 8]])
    w = [2, 1, 3, 2]
    out = coverage_difference(a, b, w, 100.0, levels=(0.25, 0.5, 1.0))
    assert len(out) == 2 and set(out[0]) == {'mean', 'quantiles', 'p_a_larger', 'p_b_larger'}
    # output 0: sum w d = 4 - 3 + 0 - 6 = -5 over W = 8; sorted d: -3 (w 1 + 2), 0 (w 3), 2 (w 2);
    # cumulative weight 3, 6, 8 against p W = 2, 4, 8 -> -3, 0, 2
    assert out[0]['mean'] == -5.0 / 8.0 * 100.0
    assert out[0]['quantiles'] == [-300.0, 0.0, 200.0]
    assert out[0]['p_a_larger'] == 2.0 / 8.0 and out[0]['p_b_larger'] == 3.0 / 8.0       # the tie counts for neither
    assert out[1] == {'mean': 100.0, 'quantiles': [100.0, 100.0, 100.0], 'p_a_larger': 1.0, 'p_b_larger': 0.0}
    # a member of weight 0 changes nothing
    again = coverage_difference(np.vstack([a, [[99, 0]]]), np.vstack([b, [[0, 99]]]), w + [0], 100.0, (0.25, 0.5, 1.0))
    assert again == out
    with pytest.raises(ValueError, match='nothing accumulated'):
        coverage_difference(a, b, [0, 0, 0, 0], 100.0)
    with pytest.raises(ValueError, match='nothing accumulated'):
        coverage_difference(np.zeros((0, 2)), np.zeros((0, 2)), [], 100.0)
    with pytest.raises(ValueError, match='cell counts'):
        coverage_difference(a, b[:3], w, 100.0)
    with pytest.raises(ValueError):
        coverage_difference(a, b, w, 100.0, levels=(0.0,))


@pytest.mark.parametrize('thr, match', [([1, 2, 3, 4, 5], 'at most 4'), ([0.0], 'finite and > 0'), ([-1.0], 'finite and > 0'),
                                        ([np.inf], 'finite and > 0'), ([np.nan], 'finite and > 0'),
                                        ([1.0, 1.0], 'strictly increasing'), ([2.0, 1.0], 'strictly increasing'),
                                        (['x'], 'must be numbers'), (3.0, 'must be numbers')])
def test_bad_contrast_thresholds_are_refused(thr, match):
    from parasitoids_amd.predictive import check_contrast_thresholds
    with pytest.raises(ValueError, match=match):
        check_contrast_thresholds(thr)


def test_good_contrast_thresholds_pass():
    from parasitoids_amd.predictive import check_contrast_thresholds
    assert check_contrast_thresholds(()) == [] and check_contrast_thresholds([1, 10]) == [1.0, 10.0]
    assert check_contrast_thresholds((1e-3, 1, 10, 100)) == [1e-3, 1.0, 10.0, 100.0]


def _model(ndays=6, R=64):
    """what the checks read of a PopModel"""
    return types.SimpleNamespace(rad_dist=10000.0, rad_res=R, days=list(range(100, 100 + ndays)), r_number=130000,
                                 prob_model=False, device=None)


def test_the_compare_argument_of_posterior_predictive():
    from parasitoids_amd.predictive import contrast_plan
    plan_a = dict(sites=[(0, 0, 0.6), (2000, 0, 0.4)], days=[0, 2, 5])
    sites, days, lags = contrast_plan(dict(sites=[(0, 0, 1.0), (0, -2000, 0.5, 4)]), plan_a, _model())
    assert days == [0, 2, 5] and lags == [0, 4] and [s['drow'] for s in sites] == [0, 13]      # plan A's days
    assert contrast_plan(dict(sites=[(0, 0, 1)]), dict(sites=[(0, 0, 2)]))[1] is None           # no model yet
    assert contrast_plan(dict(sites=[(0, 0, 1)]), dict(sites=[(0, 0, 2)]), _model())[1] == list(range(6))
    for bad, a, match in (([(0, 0, 1)], plan_a, 'compare must be dict'),
                          (dict(sites=[(0, 0, 1)], days=[0, 1]), plan_a, 'compare must be dict'),
                          (dict(), plan_a, 'compare must be dict'),
                          (dict(sites=[(0, 0, 1)]), None, 'give sites= too'),
                          (dict(sites=[(0, 0, 1)]), dict(sites=[]), 'release sites'),
                          (dict(sites=[(0, 0, -1.0)]), plan_a, 'amount'),
                          (dict(sites=[(0, 0, 1, 1)]), plan_a, 'smallest lag'),
                          (dict(sites=[(0, 0, 1), (0, 0, 1, 6)]), plan_a, "beyond the model's 6 days"),
                          (dict(sites=[(0, 0, 1), (0, 0, 1, 3)]), dict(sites=[(0, 0, 1)], days=[0, 2]),
                           'beyond the last output day'),
                          (dict(sites=[(20200.0, 0, 1)]), plan_a, 'beyond the 129 x 129 domain')):
        with pytest.raises(ValueError, match=match):
            contrast_plan(bad, a, _model())


def test_posterior_predictive_refuses_a_bad_compare_before_evaluating():
    from parasitoids_amd.predictive import posterior_predictive
    calls = []
    trace = np.zeros((3, 1))

    def evaluate(theta):
        calls.append(theta)
        return None
    good = dict(sites=[(0, 0, 1.0)])
    with pytest.raises(ValueError, match='give sites= too'):
        posterior_predictive(None, (trace, ['x']), evaluate=evaluate, compare=good)
    with pytest.raises(ValueError, match='give sites= too'):
        posterior_predictive(_model(), (trace, ['x']), evaluate=evaluate, compare=good)
    for compare in ([(0, 0, 1)], dict(sites=[]), dict(sites=[(0, 0, 0.0)]), dict(sites=[(0, 0, 1)], days=[0])):
        with pytest.raises(ValueError, match='compare must be|release sites|amount'):
            posterior_predictive(None, (trace, ['x']), evaluate=evaluate, sites=good, compare=compare)
    with pytest.raises(ValueError, match="beyond the model's 6 days"):
        posterior_predictive(_model(), (trace, ['x']), evaluate=evaluate, sites=good,
                             compare=dict(sites=[(0, 0, 1), (0, 0, 1, 7)]))
    # the run's thresholds become the contrast's: they have to be > 0 and increasing
    for thr in ((0.0,), (10.0, 1.0)):
        with pytest.raises(ValueError, match='finite and > 0|strictly increasing'):
            posterior_predictive(None, (trace, ['x']), evaluate=evaluate, sites=good, compare=good, thresholds=thr)
    assert not calls


def test_compare_sites_needs_sites_on_the_command_line():
    """refused by the argument parser, before the package is imported"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'run_predictive.py'), '--synthetic',
                        '--compare-sites', '0,0,1.5'], capture_output=True, text=True)
    assert r.returncode == 2 and '--compare-sites' in r.stderr and '--sites' in r.stderr


def test_the_contrast_entry_points_are_declared_and_bound():
    from parasitoids_amd import _lib
    names = {'ps_contrast_' + n for n in ('create', 'add_sites', 'add_project', 'merge', 'info', 'fetch', 'fetch_counts',
                                          'fetch_coverage', 'reset', 'prof', 'destroy')}
    assert names <= set(_lib.SIGNATURES)
    header = open(os.path.join(ROOT, 'include', 'parasitoid_hip.h')).read()
    lib = _lib.load()
    for n in names:
        assert n + '(' in header and hasattr(lib, n), n
