"""CPU tests of the reweighted excursion regions: the numpy reference (wexcur_ref) against the integer reference
(excur_ref) where the two must agree bit for bit -- equal log-weights, and members dropped by a log-weight of -inf --
and the argument checks that need no device: the maps option, the driver's and the script's refusals, the member
weights."""
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import excur_ref as R
import wexcur_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (9, 13)
T = 1.0


def _fields(seed, members=7):
    """random small fields around the threshold, member 2 empty (below t everywhere) and member 4 full"""
    rng = np.random.default_rng(seed)
    X = rng.lognormal(0.0, 1.5, size=(members,) + SHAPE)
    X[2] = 0.0
    X[4] = 50.0
    return X


def _same_maps(got, want):
    for name in ('above', 'below', 'contour'):
        assert got[name].dtype == np.float64 and np.array_equal(got[name], want[name]), name


@pytest.mark.parametrize('level', [0.0, -700.0])
@pytest.mark.parametrize('seed', [1, 2, 3])
def test_with_equal_log_weights_wexcur_ref_is_excur_ref(seed, level):
    X = _fields(seed)
    n = [1, 3, 1, 2, 1, 4, 2]
    want = R.plane(X, n, T)
    got = WR.plane(X, n, [level] * len(n), T)
    assert got['w'].tolist() == [float(v) for v in n] and got['W'] == float(sum(n))
    assert got['C'].dtype == np.float64 and np.array_equal(got['C'], want['C'].astype(np.float64))
    assert np.array_equal(got['hi'], want['hi'].astype(np.float64))
    lo = np.where(want['lo'] == R.NONE, np.inf, want['lo'].astype(np.float64))
    assert np.array_equal(got['lo'], lo)
    assert got['lo'][2] == np.inf and got['hi'][4] == 0.0      # the empty and the full member
    _same_maps(got, want)
    assert np.array_equal(got['prob'], want['C'] / float(sum(n)))
    assert 0.0 < got['above'].max() and got['contour'].min() < 1.0     # the planes are not trivial


@pytest.mark.parametrize('dropped', [[0], [1, 5], [2, 4, 6]])
def test_members_at_minus_infinity_drop_out(dropped):
    X = _fields(11)
    n = [1, 3, 1, 2, 1, 4, 2]
    lw = [(-math.inf if m in dropped else 0.0) for m in range(len(n))]
    keep = [m for m in range(len(n)) if m not in dropped]
    want = R.plane(X[keep], [n[m] for m in keep], T)
    got = WR.plane(X, n, lw, T)
    assert got['W'] == float(sum(n[m] for m in keep))
    assert np.array_equal(got['C'], want['C'].astype(np.float64))
    _same_maps(got, want)
    # a dropped member keeps its mask and its bounds on the others' counts
    for m in dropped:
        b = got['B'][m]
        assert got['w'][m] == 0.0
        assert got['lo'][m] == (got['C'].ravel()[b].min() if b.any() else np.inf)


def test_real_weights_move_the_maps_and_stay_in_range():
    X = _fields(5)
    n = [1, 3, 1, 2, 1, 4, 2]
    lw = [0.0, -3.5, -0.25, -8.0, -1.0, -0.5, -2.0]
    got = WR.plane(X, n, lw, T)
    plain = R.plane(X, n, T)
    assert got['W'] == WR.total(got['w']) and got['w'][0] == 1.0
    for name in ('above', 'below', 'contour', 'prob'):
        assert np.all(got[name] >= 0.0) and np.all(got[name] <= 1.0), name
    assert np.all(got['above'] <= got['prob']) and np.all(got['below'] <= 1.0 - got["prob"] + 1e-12)
    assert not np.array_equal(got['above'], plain['above'])


def test_the_maps_option_takes_excursion_last():
    from parasitoids_amd import predictive as PR
    assert PR.REWEIGHT_MAPS[-1] == 'excursion'
    assert PR.check_reweight_maps(['excursion', 'quantiles']) == ('quantiles', 'excursion')
    assert PR.check_reweight_maps(['excursion']) == ('excursion',)
    with pytest.raises(ValueError, match='maps'):
        PR.check_reweight_maps(['excursion', 'excursion'])
    with pytest.raises(ValueError, match='maps'):
        PR.check_reweight_maps('excursion')


def test_the_driver_refuses_the_option_without_excursion_before_any_chain():
    from parasitoids_amd import predictive as PR
    pm = types.SimpleNamespace(days=list(range(6)), rad_dist=10000.0, rad_res=64, device=None)
    chains = object()                    # never looked at
    rw = {'a': dict(log_weights=[np.zeros(4)]), 'options': dict(maps=('excursion',))}
    with pytest.raises(ValueError, match="maps='excursion'"):
        PR.posterior_predictive(pm, chains, reweight=rw)
    with pytest.raises(ValueError, match="maps='excursion'"):
        PR.posterior_predictive(pm, chains, reweight=rw, arrival=[1.0], quantiles=[0.5])
    # nothing is kept or built without the option
    fs = PR._FieldSet()
    res = PR.PredictiveResult(None, 0, 0, 0, 0.0, [], None, [], None)
    assert fs.reweight_excursion is None and fs._rw_lam is None and res.reweight_excursion is None


def test_the_script_refuses_excursion_without_its_maps():
    """refused by the argument parser, before the package is imported"""
    script = os.path.join(ROOT, 'scripts', 'run_predictive.py')
    rw = ['--reweight', 'a:0,0,1,none,1']
    for flags, message in ((rw + ['--reweight-maps', 'excursion'], 'give --excursion too'),
                           (rw + ['--reweight-maps', 'quantiles,excursion', '--quantiles', '0.5'], 'give --excursion too'),
                           (rw + ['--reweight-maps', 'excursion,peak', '--excursion', '1'], 'takes a subset')):
        r = subprocess.run([sys.executable, script, '--synthetic'] + flags, capture_output=True, text=True)
        assert r.returncode == 2 and message in r.stderr, (flags, r.stderr[-300:])
        assert 'Traceback' not in r.stderr


def test_the_member_weights_and_their_refusals():
    from parasitoids_amd import predictive as PR
    n = [1, 3, 2]
    w = PR.excursion_member_weights([-1.0, 0.5, -math.inf], n)
    assert w.dtype == np.float64 and w.tolist() == [1 * math.exp(-1.5), 3.0, 0.0]
    assert np.array_equal(w, WR.member_weights(n, [-1.0, 0.5, -math.inf]))
    assert PR.excursion_member_weights([-700.0] * 3, n).tolist() == [1.0, 3.0, 2.0]
    for bad, message in (([0.0, 0.0], 'members'), ([0.0, 0.0, 0.0, 0.0], 'members'), ([0.0, math.nan, 0.0], 'NaN'),
                         ([0.0, math.inf, 0.0], 'NaN'), ([-math.inf] * 3, '-inf')):
        with pytest.raises(ValueError, match=message):
            PR.excursion_member_weights(bad, n)
    # the class checks its parent before anything touches the device
    with pytest.raises(ValueError, match='ExcursionMaps'):
        PR.ReweightedExcursion(object(), [0.0])


def test_the_new_entry_points_are_declared_and_bound():
    from parasitoids_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'parasitoid_hip.h')).read()
    for n in ('create', 'plane', 'fetch_counts', 'fetch_bounds', 'map', 'member_weights', 'info', 'prof', 'destroy'):
        assert 'ps_wexcur_' + n in _lib.SIGNATURES and 'ps_wexcur_' + n + '(' in header, n
    makefile = open(os.path.join(ROOT, 'parasitoids_amd', 'csrc', 'Makefile')).read()
    assert ' ps_wexcur.hip' in makefile
