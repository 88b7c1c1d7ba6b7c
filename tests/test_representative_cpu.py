"""CPU tests of the representative members (predictive.inclusion_depth, median_member, central_members,
set_distance, k_medoids, check_representative): the host functions against the loop reference (overlap_ref) on
random bit sets, hand-made cases with known depths, medians and scenarios, PAM against the exhaustive optimum, and
the refusals of posterior_predictive(representative=...) before any evaluation.  Integers everywhere: every
comparison is exact."""
import numpy as np
import pytest

from parasitoids_amd import _lib as L
from parasitoids_amd import predictive as PP

import overlap_ref as R


def _sets(rows, ncell=None):
    """[M, ncell] bool from lists of cell indices"""
    ncell = ncell or 1 + max(max(r) for r in rows if len(r))
    B = np.zeros((len(rows), ncell), dtype=bool)
    for m, r in enumerate(rows):
        B[m, list(r)] = True
    return B


def _check(B, w, eps, cen=0.5, K=None):
    """the host functions on the table of B against the reference -> (depth, scenarios)"""
    I = R.table(B)
    M = len(w)
    e, c = int(round(1000 * eps)), int(round(1000 * cen))
    d, w_in, w_cont = R.depth(I, w, e)
    got = PP.inclusion_depth(I.astype(np.uint32), np.asarray(w, dtype=np.uint32), eps)
    assert all(g.dtype == np.int64 for g in got)
    assert got[0].tolist() == d and got[1].tolist() == w_in and got[2].tolist() == w_cont
    assert all(int(w[i]) <= d[i] <= sum(w) for i in range(M))
    assert PP.median_member(got[0]) == R.median(d)
    assert PP.central_members(got[0], w, cen) == R.central(d, w, c)
    D = PP.set_distance(I)
    assert D.dtype == np.int64 and D.tolist() == R.distance(I)
    assert np.array_equal(D, (B[:, None, :] != B[None, :, :]).sum(2))
    K = min(M, 3) if K is None else K
    want = R.k_medoids(R.distance(I), w, K)
    sc = PP.k_medoids(D, w, K)
    assert sc['medoids'] == want['medoids'] and list(sc['assignment']) == want['assignment']
    assert sc['cluster_weight'] == want['cluster_weight'] and sc['cost'] == want['cost']
    assert sc['costs_by_k'] == want['costs_by_k'] and sc['cost'] == want['costs_by_k'][-1]
    assert sum(sc['cluster_weight']) == sum(w)
    return d, sc


@pytest.mark.parametrize('M', [1, 2, 7, 40])
@pytest.mark.parametrize('eps', [0.0, 0.02, 0.5])
def test_host_functions_match_the_loop_reference_on_random_sets(M, eps):
    rng = np.random.default_rng(100 * M + int(1000 * eps))
    # members of very different sizes, so that inclusions do happen: each a random subset of a random-size prefix
    B = np.array([(rng.random(130) < rng.random()) & (np.arange(130) < rng.integers(1, 131)) for _ in range(M)])
    w = rng.integers(1, 6, M).tolist()
    for cen in (0.5, 0.001, 1.0):
        _check(B, w, eps, cen)
    if M <= 7:
        for K in range(1, M + 1):
            _d, sc = _check(B, w, eps, K=K)
            assert sc['cost'] >= R.exhaustive(R.distance(R.table(B)), w, K)
        assert sc['cost'] == 0 and sorted(sc['medoids']) == list(range(M))            # K = M


def test_a_nested_chain_has_the_known_depths_and_the_middle_median():
    B = _sets([range(n) for n in (2, 5, 9, 14, 20)])
    d, _sc = _check(B, [1] * 5, 0.0)
    assert d == [1, 2, 3, 2, 1] and PP.median_member(np.array(d)) == 2
    assert PP.central_members(np.array(d), [1] * 5, 0.5) == [2, 1, 3]              # 3 of 5 is the first >= half
    assert PP.central_members(np.array(d), [1] * 5, 0.2) == [2]
    assert PP.central_members(np.array(d), [1] * 5, 1.0) == [2, 1, 3, 0, 4]
    d3, _sc = _check(B, [1, 1, 3, 1, 1], 0.0)
    assert d3 == [1, 2, 5, 2, 1]                                                    # in: 7 6 5 2 1; cont: 1 2 5 6 7


def test_a_disjoint_outlier_has_its_own_weight_as_depth():
    B = _sets([range(0, 10), range(0, 12), range(2, 9), range(50, 60)])
    w = [2, 1, 3, 4]
    d, sc = _check(B, w, 0.02, K=2)
    assert d[3] == 4 and all(x > 0 for x in d[:3])
    assert sc['medoids'] == [2, 3] and sc['cost'] == 11 and sc['cluster_weight'] == [6, 4]
    assert list(sc['assignment']) == [0, 0, 0, 1]


def test_duplicates_tie_and_the_smallest_index_wins():
    B = _sets([range(0, 6), range(0, 9), range(0, 9), range(0, 12)])
    d, sc = _check(B, [1, 1, 1, 1], 0.0, K=1)
    assert d == [1, 3, 3, 1] and PP.median_member(np.array(d)) == 1
    assert PP.central_members(np.array(d), [1] * 4, 0.5) == [1, 2]
    assert sc['medoids'] == [1]                                                     # members 1 and 2 cost the same


def test_a_stray_cell_is_included_from_one_nth_on():
    n = 50                                           # 49 cells inside the big set and one stray: out = 1, n = 50
    B = _sets([list(range(49)) + [99], range(0, 99)], 100)    # the big set never lies in the small one: 50 of 99 out
    for eps, inside in ((0.019, False), (0.02, True), (0.021, True), (0.0, False), (0.5, True)):
        d, w_in, w_cont = PP.inclusion_depth(R.table(B), [1, 1], eps)
        assert w_in.tolist() == ([2, 1] if inside else [1, 1]), eps
        assert w_cont.tolist() == ([1, 2] if inside else [1, 1]), eps
        assert (1000 * 1 <= int(round(1000 * eps)) * n) == inside
        _check(B, [1, 1], eps)


def test_two_well_separated_groups_are_recovered():
    near = [range(0, 20), range(0, 22), range(1, 21), range(0, 19)]
    far = [range(100, 130), range(101, 131), range(100, 128)]
    B = _sets(near + far, 140)
    w = [1, 2, 1, 1, 2, 1, 1]
    _d, sc = _check(B, w, 0.02, K=2)
    D = R.distance(R.table(B))
    want = R.k_medoids(D, w, 2)
    assert sc['medoids'] == want['medoids'] == [0, 4]
    assert list(sc['assignment']) == [0, 0, 0, 0, 1, 1, 1] and sc['cluster_weight'] == [5, 4]
    for K in (1, 2):
        assert PP.k_medoids(PP.set_distance(R.table(B)), w, K)['cost'] == R.exhaustive(D, w, K)   # hand-made: the optimum
    full = PP.k_medoids(PP.set_distance(R.table(B)), w, 7)
    assert all(a >= b for a, b in zip(full['costs_by_k'], full['costs_by_k'][1:])) and full['cost'] == 0
    assert full['costs_by_k'][:2] == [R.exhaustive(D, w, 1), R.exhaustive(D, w, 2)]


def test_all_empty_sets():
    B = np.zeros((4, 70), dtype=bool)
    w = [1, 2, 3, 1]
    d, sc = _check(B, w, 0.02, K=2)
    assert d == [7, 7, 7, 7] and PP.median_member(np.array(d)) == 0
    assert not PP.set_distance(R.table(B)).any() and sc['cost'] == 0 and sc['costs_by_k'] == [0, 0]


def _chain():
    from parasitoids_amd import mcmc
    names = [m[0] for m in mcmc.MODEL_BLOCK]
    t0 = np.array([m[2] for m in mcmc.MODEL_BLOCK])
    return np.array([t0, t0, t0 * 1.01]), names


@pytest.mark.parametrize('arg', [dict(epsilon=0.0205), dict(epsilon=0.6), dict(epsilon=-0.001), dict(central=0),
                                 dict(central=1.001), dict(central=0.3333), dict(clusters=9), dict(clusters=0),
                                 dict(clusters=2.5), dict(days=[]), dict(days=[1, 1]), dict(days='some'),
                                 dict(cluster=2), 'yes'])
def test_bad_settings_raise(arg):
    with pytest.raises(ValueError):
        PP.check_representative(arg)
    with pytest.raises(ValueError) as err:         # and before any evaluation: there is no model either
        PP.posterior_predictive(None, _chain(), excursion=[1, 10], representative=arg)
    assert 'PopModel' not in str(err.value)


def test_the_refusals_the_defaults_and_the_library_symbols():
    assert PP.check_representative(True) == dict(epsilon=0.02, central=0.5, clusters=3, days='all')
    got = PP.check_representative(dict(epsilon=0.1, days=(2, 0)))
    assert got == dict(epsilon=0.1, central=0.5, clusters=3, days=[2, 0])
    with pytest.raises(ValueError, match='excursion'):
        PP.posterior_predictive(None, _chain(), representative=True)
    calls = []

    def evaluate(theta):
        calls.append(theta)
        return True
    with pytest.raises(ValueError, match='evaluate'):
        PP.posterior_predictive(None, _chain(), evaluate=evaluate, representative=True)
    assert calls == []
    with pytest.raises(ValueError, match='PopModel'):   # good arguments get as far as the missing model
        PP.posterior_predictive(None, _chain(), excursion=[1, 10], representative=dict(clusters=2))
    res = PP.posterior_predictive(None, _chain(), evaluate=evaluate)
    assert res.representative is None and res.representative_days is None
    for bad in (lambda: PP.inclusion_depth(np.zeros((2, 3)), [1, 1], 0.0),
                lambda: PP.inclusion_depth(np.zeros((2, 2)), [1, 0], 0.0),
                lambda: PP.inclusion_depth(np.zeros((2, 2)), [1, 1], 0.0205),
                lambda: PP.central_members(np.array([1, 1]), [1, 1], 0),
                lambda: PP.k_medoids(np.zeros((2, 2)), [1, 1], 3),
                lambda: PP.k_medoids(np.zeros((2, 2)), [1, 1], 9),
                lambda: PP.MemberOverlap(object())):
        with pytest.raises(ValueError):
            bad()
    for name in ('create', 'pairs', 'subset', 'info', 'prof', 'destroy'):
        assert 'ps_overlap_' + name in L.SIGNATURES
