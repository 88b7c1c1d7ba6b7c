"""Host-side tests of the neighbourhood maps (predictive.NeighbourhoodFields and its helpers): the metres -> r2 rule,
the argument checks and the parser, the numpy restatement (nbhd_ref) against scipy's maximum filter, the driver's
request check, and that nothing is built where nothing is asked for."""
import math
import os
import types

import numpy as np
import pytest

import nbhd_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_cells_counts_the_cells_of_the_disc():
    from parasitoids_amd.predictive import window_cells
    for r2, n in ((0, 1), (1, 5), (2, 9), (4, 13), (5, 21), (25, 81)):
        got = window_cells(25.0 * math.sqrt(r2) * (1 + 1e-12), 25.0)
        assert got == (r2, math.isqrt(r2), n), (r2, got)
        assert len(nbhd_ref.disc_offsets(r2)) == n and nbhd_ref.disc_footprint(r2).sum() == n
        assert nbhd_ref.window_cells(25.0 * math.sqrt(r2) * (1 + 1e-12), 25.0) == got
    # just below a radius the smaller disc
    assert window_cells(25.0 * math.sqrt(5) * (1 - 1e-6), 25.0)[0] == 4
    assert window_cells(0.0, 25.0) == (0, 0, 1)


def test_a_radius_of_whole_cells_keeps_its_square():
    from parasitoids_amd.predictive import window_cells
    for cell in (25.0, 10000.0 / 400, 10000.0 / 512, 10000.0 / 2048):
        for k in range(1, 33):
            r2, H, n = window_cells(k * cell, cell)
            assert (r2, H) == (k * k, k), (cell, k, r2)
            assert nbhd_ref.window_cells(k * cell, cell) == (r2, H, n)


def test_radii_beyond_the_largest_disc_are_refused():
    from parasitoids_amd.predictive import window_cells
    assert window_cells(32.99 * 25.0, 25.0)[1] == 32
    for radius in (33 * 25.0, 1e4, 1e300):
        with pytest.raises(ValueError, match='825 m'):         # names the largest radius of this grid
            window_cells(radius, 25.0)
    for radius in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            window_cells(radius, 25.0)


def test_check_windows_and_the_parser():
    from parasitoids_amd.predictive import check_windows, parse_windows
    assert check_windows([(1, 0), (3, 200.0), [5, 400]]) == [(1, 0.0), (3, 200.0), (5, 400.0)]
    assert check_windows([(0, 1.5)] * 32) == [(0, 1.5)] * 32
    bad = [[], [(0, 1.0)] * 33, 5, [(1,)], [(1, 2.0, 3)], [('a', 1.0)], [(1.5, 1.0)], [(-1, 1.0)], [(1, -1.0)],
           [(1, float('nan'))], [(1, float('inf'))], [(float('inf'), 1.0)], [(1, None)], [5]]
    for arg in bad:
        with pytest.raises(ValueError):
            check_windows(arg)
    with pytest.raises(ValueError, match='output'):
        check_windows([(1.5, 1.0)], 'output')
    assert parse_windows('5,100;5,200.5; 17 , 800 ;') == [(5, 100.0), (5, 200.5), (17, 800.0)]
    for text in ('5', '5,1,2', 'a,1', '5,x', '2.5,1'):
        with pytest.raises(ValueError):
            parse_windows(text)
    src = open(os.path.join(ROOT, 'scripts', 'run_predictive.py')).read()
    for flag in ('--neighbourhood', 'nbhd_ms_per_member', 'nbhd_projection_ms_per_member'):
        assert flag in src


@pytest.mark.parametrize('N', [5, 33, 67, 129])
def test_the_restatement_against_scipy(N):
    from scipy import ndimage
    rng = np.random.default_rng(N)
    v = np.where(rng.random((N, N)) < 0.02, rng.random((N, N)) * 1e3, 0.0)
    v[0, 0], v[N - 1, N - 1], v[0, N // 2] = 3.0, 7.0, 11.0
    for r2 in (0, 1, 2, 5, 25, 169, 1024):              # N = 5 and 33 are smaller than the largest discs
        want = ndimage.maximum_filter(v, footprint=nbhd_ref.disc_footprint(r2), mode='constant', cval=-np.inf)
        got = nbhd_ref.neighbourhood_max(v, r2)
        assert np.array_equal(got, want), (N, r2)
        assert (got >= v).all()
    assert np.array_equal(nbhd_ref.neighbourhood_max(v, 0), v)
    # negative values: nothing outside the domain wins the maximum
    w = -1.0 - rng.random((N, N))
    assert np.array_equal(nbhd_ref.neighbourhood_max(w, 25),
                          ndimage.maximum_filter(w, footprint=nbhd_ref.disc_footprint(25), mode='constant',
                                                 cval=-np.inf))
    assert (nbhd_ref.neighbourhood_max(w, 25) < 0).all()


def test_check_neighbourhood():
    from parasitoids_amd.predictive import check_neighbourhood
    got = check_neighbourhood([(1, 0), (3, 200.0)], 6, 25.0)
    assert got == {'windows': [(1, 0.0), (3, 200.0)], 'given': [[1, 0.0], [3, 200.0]]}
    assert check_neighbourhood(dict(windows=[(5, 800)]), 6, 25.0)['windows'] == [(5, 800.0)]
    assert check_neighbourhood([(5, 8000)], 6)['windows'] == [(5, 8000.0)]      # no grid at hand: the model's check
    for arg in ([(6, 1.0)], [(1, 825.0)], dict(), dict(windows=[(1, 1.0)], other=1), dict(radius=3), [], None,
                [(d, 1.0) for d in range(33)]):
        with pytest.raises(ValueError):
            check_neighbourhood(arg, 6, 25.0)
    with pytest.raises(ValueError, match='evaluate'):
        check_neighbourhood([(1, 1.0)], 6, 25.0, evaluate=lambda theta: None)


def test_posterior_predictive_refuses_before_any_evaluation():
    from parasitoids_amd.predictive import posterior_predictive
    calls = []

    def evaluate(theta):
        calls.append(theta)
        return None
    chain = (np.zeros((3, 1)), ['x'])
    with pytest.raises(ValueError, match='evaluate'):
        posterior_predictive(None, chain, evaluate=evaluate, neighbourhood=[(1, 100.0)])
    with pytest.raises(ValueError, match='radius'):
        posterior_predictive(None, chain, neighbourhood=[(1, -100.0)])
    with pytest.raises(ValueError, match='windows'):
        posterior_predictive(None, chain, neighbourhood=dict(days=[1]))
    pm = types.SimpleNamespace(days=list(range(6)), rad_dist=10000.0, rad_res=400)
    with pytest.raises(ValueError, match='6 days'):
        posterior_predictive(pm, chain, neighbourhood=[(6, 100.0)])
    with pytest.raises(ValueError, match='825 m'):
        posterior_predictive(pm, chain, neighbourhood=dict(windows=[(1, 900.0)]))
    assert not calls


def test_without_neighbourhood_nothing_is_built():
    from parasitoids_amd import predictive as PR
    for kind in ('days', 'sites'):
        assert 'neighbourhood' in PR.FEED_ORDER[kind]
    assert 'neighbourhood' not in PR.FEED_ORDER['projection'] and 'neighbourhood' not in PR.FEED_ORDER['compare']
    assert 'neighbourhood' in PR.ACCUMULATORS and 'neighbourhood' in PR.BUILD
    q = types.SimpleNamespace(nb_plan=None)
    fs = PR._FieldSet().fed_from('days', object(), owns=False, catch=None, information=None, neighbourhood=None)
    assert PR.BUILD['neighbourhood'](fs, q) is None and fs.neighbourhood is None
    fs = PR._FieldSet().fed_from('days', object(), owns=False)                  # the key left out altogether
    assert PR.BUILD['neighbourhood'](fs, q) is None
    # the request of a call without the argument carries no plan, and the result no maps
    chain = (np.zeros((3, len(PR.model_names()))), PR.model_names())
    res = PR.posterior_predictive(None, chain, evaluate=lambda theta: None)
    assert res.neighbourhood is None
    assert PR.NeighbourhoodFields.fields_kind == 'nbhd' and PR.NeighbourhoodFields._prefix == 'ps_nbhd'
