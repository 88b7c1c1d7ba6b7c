"""CPU tests of the joint excursion sets (predictive.ExcursionMaps, ps_excur_*): the numpy reference on hand-made
members (nested members: joint == marginal; crossing members: joint < marginal on the symmetric difference; an
empty member, a member above t everywhere, C = W / 2) and on random fields (the inequalities against the marginal
probability, monotonicity in C, a brute-force check over every level set, invariance under permuting the members),
the argument checks of ExcursionMaps and of posterior_predictive(excursion=...) before any evaluation, and the
result file of save_excursion."""
import json

import numpy as np
import pytest

from parasitoids_amd import predictive as PP

import excur_ref as R


def _plane(masks, weights):
    """the reference of members given as 0 / 1 rows, at t = 1"""
    return R.plane(np.array(masks, dtype=np.float64), weights, 1.0)


# ------------------------------------------------------------------ the numpy reference, by hand
def test_three_nested_members_give_joint_equal_marginal():
    P = _plane([[1, 1, 1, 1, 0, 0], [1, 1, 1, 0, 0, 0], [1, 0, 0, 0, 0, 0]], [1, 2, 3])
    W = 6.0
    assert P['C'].tolist() == [6, 3, 3, 1, 0, 0]
    assert P['hi'].tolist() == [0, 1, 3] and P['lo'].tolist() == [1, 3, 6]
    Ap, Am, Ac = R.numerators(P['C'].ravel(), P['hi'], P['lo'], [1, 2, 3])
    assert np.array_equal(Ap, P['C']) and np.array_equal(Am, 6 - P['C'])   # every level set is some member's mask
    assert np.array_equal(P['above'], P['C'] / W)
    assert Ac.tolist() == [6, 0, 0, 5, 6, 6]                       # C = 3 = W / 2: nothing; C = 1: the members with lo > 1
    assert P['contour'].tolist() == [1.0, 0.0, 0.0, 5 / W, 1.0, 1.0]
    assert R.region(P['above'], P['below'], 0.6).tolist() == [1, 0, 0, -1, -1, -1]


def test_two_crossing_members_give_joint_below_marginal_on_the_symmetric_difference():
    P = _plane([[1, 1, 0, 0], [1, 0, 1, 0]], [1, 1])
    assert P['C'].tolist() == [2, 1, 1, 0]
    assert P['hi'].tolist() == [1, 1] and P['lo'].tolist() == [1, 1]
    assert P['above'].tolist() == [1.0, 0.0, 0.0, 0.0]              # marginal 0.5 on cells 1 and 2, joint 0
    assert P['below'].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert P['contour'].tolist() == [1.0, 0.0, 0.0, 1.0]            # C = W / 2 gives Fc = 0
    marginal = P['C'] / 2.0
    sym = np.array([False, True, True, False])
    assert np.all(P['above'][sym] < marginal[sym]) and np.all(P['above'][~sym] == marginal[~sym])


def test_an_empty_member_and_a_member_above_everywhere_take_the_sentinels():
    P = _plane([[0, 0, 0, 0], [1, 1, 1, 0], [1, 1, 0, 0]], [2, 1, 1])
    assert P['lo'][0] == R.NONE == 0xffffffff and P['hi'][0] == 2
    assert P['below'][3] == 1.0                                     # nobody holds anything there
    assert P['words'].dtype == np.dtype('<u8') and P['words'].shape == (3, 1)
    assert P['words'][:, 0].tolist() == [0, 7, 3]                   # little-endian bits, 60 pad bits 0
    Q = _plane([[1, 1, 1], [1, 0, 0]], [3, 1])
    assert Q['hi'][0] == 0 and Q['lo'][0] == 3                      # above t everywhere: no cell outside
    assert Q['above'].tolist() == [1.0, 0.75, 0.75] and Q['below'].tolist() == [0.0, 0.25, 0.25]
    Z = _plane([[0, 0], [0, 0]], [1, 1])                            # no member holds anything anywhere
    assert Z['hi'].tolist() == [0, 0] and Z['lo'].tolist() == [R.NONE] * 2
    assert Z['above'].tolist() == [0.0, 0.0] and Z['below'].tolist() == [1.0, 1.0] and Z['contour'].tolist() == [1.0, 1.0]


def test_the_pad_of_the_last_word_stays_zero():
    B = np.ones((2, 65), dtype=bool)
    w = R.pack(B)
    assert w.shape == (2, 2) and w[0, 0] == 0xffffffffffffffff and w[0, 1] == 1


# ------------------------------------------------------------------ the numpy reference, random fields
def _random_planes():
    rng = np.random.default_rng(5)
    members = [10 ** rng.uniform(-2, 2, size=(7, 300)) * (rng.random((7, 300)) > 0.35) for _ in range(6)]
    weights = [1, 3, 1, 2, 1, 4]
    # members that overlap a lot: a common plume scaled per member, so that level sets are often covered jointly
    plume = 10 ** rng.uniform(-1, 2, size=(7, 300))
    for m in range(3):
        members[m] = plume * (0.5 + 0.4 * m) * (rng.random((7, 300)) > 0.02)
    return members, weights


@pytest.mark.parametrize('t', [1.0, 10.0])
def test_identities_on_random_fields(t):
    members, weights = _random_planes()
    W = sum(weights)
    strict = 0
    for s in range(7):
        X = np.array([m[s] for m in members])
        P = R.plane(X, weights, t)
        C = P['C']
        Ap, Am, Ac = R.numerators(C, P['hi'], P['lo'], weights)
        assert np.all(P['above'] <= C / W) and np.all(P['below'] <= 1.0 - C / W)
        assert np.all(Ap <= C) and np.all(Am <= W - C)
        strict += int((Ap < C).sum())
        assert np.all(Ac[2 * C > W] <= Ap[2 * C > W]) and np.all(Ac[2 * C < W] <= Am[2 * C < W])
        assert np.all(Ac[2 * C == W] == 0)
        order = np.argsort(C, kind='stable')
        assert np.all(np.diff(Ap[order]) >= 0) and np.all(np.diff(Am[order]) <= 0)
        # brute force: the weight of the members whose mask covers {C >= n}, and of those that miss {C <= n}
        w = np.asarray(weights)
        for n in np.unique(C):
            up, down = C >= n, C <= n
            cover = sum(int(w[m]) for m in range(len(w)) if P['B'][m][up].all())
            miss = sum(int(w[m]) for m in range(len(w)) if not P['B'][m][down].any())
            if n > 0:
                assert np.all(Ap[C == n] == cover), (s, n)
            assert np.all(Am[C == n] == miss), (s, n)
        # region: never both signs
        for level in (0.51, 0.75, 1.0):
            assert not np.any((P['above'] >= level) & (P['below'] >= level))
        # permuting the members permutes the bounds and changes no map
        perm = [3, 0, 5, 1, 4, 2]
        Q = R.plane(X[perm], [weights[i] for i in perm], t)
        assert np.array_equal(Q['C'], C) and np.array_equal(Q['hi'], P['hi'][perm]) and np.array_equal(Q['lo'], P['lo'][perm])
        for key in ('above', 'below', 'contour'):
            assert np.array_equal(Q[key], P[key]), key
    assert strict > 0                                               # joint < marginal somewhere: not vacuous


def test_areas_count_cells_of_the_three_sets():
    P = _plane([[1, 1, 1, 1, 0, 0], [1, 1, 1, 0, 0, 0], [1, 0, 0, 0, 0, 0]], [1, 2, 3])
    a = R.areas(P['above'], P['below'], P['contour'], [0.6, 1.0], 4.0)
    assert a == [{'level': 0.6, 'above': 4.0, 'below': 12.0, 'band': 8.0},
                 {'level': 1.0, 'above': 4.0, 'below': 8.0, 'band': 12.0}]


# ------------------------------------------------------------------ argument checks, no device
def test_check_excursion_and_levels():
    assert PP.check_excursion([1, 10]) == ([1.0, 10.0], [0.9, 0.95])
    assert PP.check_excursion(dict(thresholds=[2], levels=(0.75, 1.0))) == ([2.0], [0.75, 1.0])
    assert PP.level_tag(0.95) == 'l95' and PP.level_tag(0.975) == 'l97p5' and PP.level_tag(1.0) == 'l100'
    for bad in ([], [1, 1], [10, 1], [0, 1], [-1.0], [1, float('inf')], [1, 2, 3, 4, 5], 3.0,
                dict(thresholds=[1], levels=[0.5]), dict(thresholds=[1], levels=[0.3]), dict(thresholds=[1], levels=[1.01]),
                dict(thresholds=[1], levels=[]), dict(levels=[0.9]), dict(thresholds=[1], level=[0.9])):
        with pytest.raises(ValueError):
            PP.check_excursion(bad)


def test_class_argument_checks_come_before_the_device():
    pm = type('PM', (), {'days': list(range(40)), 'rad_res': 4, 'rad_dist': 100.0, 'device': None})()
    for thr in ([], [1, 1], [0.0], [1, 2, 3, 4, 5], [float('nan')]):
        with pytest.raises(ValueError):
            PP.ExcursionMaps(pm, thr, [0, 1])
    for days in ([], [1, 1], [2, 0], [-1, 0], list(range(33))):
        with pytest.raises(ValueError):
            PP.ExcursionMaps(pm, [1.0], days)
    with pytest.raises(ValueError):
        PP.ExcursionMaps(pm, [1.0])                                 # all 40 days: more than one launch holds
    from parasitoids_amd import _lib as L
    for name in ('create', 'reserve', 'add', 'add_project', 'add_sites', 'add_peak', 'merge', 'info', 'reset', 'finalize',
                 'map', 'fetch_counts', 'fetch_mask', 'fetch_bounds', 'prof', 'destroy'):
        assert 'ps_excur_' + name in L.SIGNATURES


def _chain():
    from parasitoids_amd import mcmc
    names = [m[0] for m in mcmc.MODEL_BLOCK]
    t0 = np.array([m[2] for m in mcmc.MODEL_BLOCK])
    return np.array([t0, t0, t0 * 1.01]), names


@pytest.mark.parametrize('kw', [dict(excursion=[10, 1]), dict(excursion=[1, 1]), dict(excursion=[0, 1]),
                                dict(excursion=[-2.0]), dict(excursion=[]), dict(excursion=[1, float('nan')]),
                                dict(excursion=[1, 2, 3, 4, 5]),
                                dict(excursion=dict(thresholds=[1], levels=[0.5])),
                                dict(excursion=dict(thresholds=[1], levels=[0.2, 0.9])),
                                dict(excursion=dict(thresholds=[1], levels=[1.5])),
                                dict(excursion=dict(threshold=[1])), dict(excursion=[1], days=[2, 0, 5]),
                                dict(excursion=[1], days=[1, 1]), dict(excursion=[1], days=list(range(33)))])
def test_bad_excursion_arguments_raise_before_any_evaluation(kw):
    with pytest.raises(ValueError) as err:
        PP.posterior_predictive(None, _chain(), **kw)     # no model either: the checks come first
    assert 'PopModel' not in str(err.value)
    with pytest.raises(ValueError, match='PopModel'):     # good arguments get as far as the missing model
        PP.posterior_predictive(None, _chain(), excursion=[1, 10], days=[0, 2, 5])


def test_excursion_is_refused_together_with_evaluate():
    calls = []

    def evaluate(theta):
        calls.append(theta)
        return True
    for exc in ([1.0, 10.0], dict(thresholds=[1.0])):
        with pytest.raises(ValueError, match='evaluate'):
            PP.posterior_predictive(None, _chain(), evaluate=evaluate, excursion=exc)
    assert calls == []
    res = PP.posterior_predictive(None, _chain(), evaluate=evaluate)
    assert res.excursion is None and res.excursion_levels is None and res.summary is None


# ------------------------------------------------------------------ result files
class _Maps():
    """what save_excursion uses of ExcursionMaps, from the numpy reference of three 5 x 5 members on two days"""
    thresholds = [1.0, 10.0]
    days = [0, 3]
    members = 3
    total_weight = 6.0
    cell_area = 25.0

    def __init__(self):
        rng = np.random.default_rng(2)
        base = 10 ** rng.uniform(-1, 2, size=(2, 5, 5))
        fields = [base * f * (rng.random((2, 5, 5)) > 0.1) for f in (0.5, 1.0, 2.0)]
        self.w = [1, 2, 3]
        self.P = {(k, d): R.plane(np.array([f[s] for f in fields]), self.w, t)
                  for k, t in enumerate(self.thresholds) for s, d in enumerate(self.days)}

    def counts(self, k, d):
        return self.P[k, d]['C'].astype(np.uint32)

    def bounds(self, k, d):
        P = self.P[k, d]
        return P['hi'].astype(np.uint32), P['lo'].astype(np.uint32), np.asarray(self.w, dtype=np.uint32)

    def above(self, k, d):
        return self.P[k, d]['above']

    def below(self, k, d):
        return self.P[k, d]['below']

    def contour(self, k, d):
        return self.P[k, d]['contour']

    def areas(self, k, d, levels):
        P = self.P[k, d]
        return R.areas(P['above'], P['below'], P['contour'], levels, self.cell_area)


def test_save_excursion_writes_the_listed_keys_and_the_json_block(tmp_path):
    from scipy import sparse
    M = _Maps()
    block = PP.save_excursion(str(tmp_path / 'd' / 'pp_excur'), M, [0.9, 0.95])
    want = {'days', 'excur_counts', 'excur_hi', 'excur_lo', 'excur_weights', 'excur_thresholds', 'excur_days'}
    want |= {'%d_%s%d_%s' % (d, n, k, t) for d in (0, 3) for n in ('above', 'below', 'contour') for k in (0, 1)
             for t in ('data', 'ind', 'indptr')}
    want |= {'%d_region%d_%s' % (d, k, tag) for d in (0, 3) for k in (0, 1) for tag in ('l90', 'l95')}
    with np.load(str(tmp_path / 'd' / 'pp_excur.npz')) as f:
        assert set(f.files) == want
        assert f['days'].tolist() == [0, 3] and f['excur_days'].tolist() == [0, 3]
        assert f['excur_thresholds'].tolist() == [1.0, 10.0] and f['excur_weights'].tolist() == [1, 2, 3]
        assert f['excur_counts'].dtype == np.uint16 and f['excur_counts'].shape == (2, 2, 5, 5)
        assert np.array_equal(f['excur_counts'][1, 0], M.counts(1, 0))
        assert f['excur_hi'].dtype == np.uint32 and f['excur_hi'].shape == (2, 2, 3)
        assert np.array_equal(f['excur_lo'][0, 1], M.bounds(0, 3)[1])
        for name, fn in (('above', M.above), ('below', M.below), ('contour', M.contour)):
            key = '3_%s1' % name
            D = sparse.csr_matrix((f[key + '_data'], f[key + '_ind'], f[key + '_indptr']), shape=(5, 5)).toarray()
            assert np.array_equal(D, fn(1, 3)), name
        reg = f['0_region0_l90']
        assert reg.dtype == np.int8 and np.array_equal(reg, R.region(M.above(0, 0), M.below(0, 0), 0.9))
        assert set(np.unique(f['3_region1_l95']).tolist()) <= {-1, 0, 1}
    assert block == {'thresholds': [1.0, 10.0], 'days': [0, 3], 'levels': [0.9, 0.95], 'members': 3,
                     'total_weight': 6.0, 'cell_area': 25.0,
                     'areas': [[{'day': d, 'levels': M.areas(k, d, [0.9, 0.95])} for d in (0, 3)] for k in range(2)]}
    json.dumps(block)
