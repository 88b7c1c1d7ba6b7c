"""CPU tests of the posterior sensitivity maps (predictive.ParamMoments / SensitivityMaps, ps_sens_*): the
scalar moments against numpy's weighted covariance, merging, the factor of a rank-deficient set, the deviation
vector against its definition, the name and limit checks, the refusal of a finalize with too few members, the
numpy replay (sens_ref) against a two-pass covariance, and argument validation before any evaluation.  No
device."""
import numpy as np
import pytest

from parasitoids_amd import mcmc
from parasitoids_amd import predictive as PP

import sens_ref

NAMES = [m[0] for m in mcmc.MODEL_BLOCK]
WEIGHTS = [1, 3, 1, 2, 1, 4, 2, 1]


def _thetas(n=8, k=4, seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, k)) * np.array([170.0, 150.0, 0.1, 1.0])[:k] + np.array([180.0, 150.0, 0.5, 1.0])[:k]


def _fill(names, T, w):
    pm = PP.ParamMoments(names)
    for t, wi in zip(T, w):
        pm.update(t, wi)
    return pm


def test_param_moments_match_numpy_weighted_covariance():
    T = _thetas()
    pm = _fill(list('abcd'), T, WEIGHTS)
    assert pm.W == sum(WEIGHTS) and pm.members == len(T)
    ref = np.cov(T.T, aweights=WEIGHTS, ddof=0)
    scale = np.sqrt(np.outer(np.diag(ref), np.diag(ref)))
    assert np.abs(pm.cov() - ref).max() <= 1e-13 * scale.max()
    assert np.all(np.abs(pm.cov() - ref) <= 1e-12 * scale)
    np.testing.assert_allclose(pm.mean(), np.average(T, axis=0, weights=WEIGHTS), rtol=1e-14)
    np.testing.assert_allclose(pm.inv_sd(), 1.0 / np.sqrt(np.diag(ref)), rtol=1e-12)
    np.testing.assert_allclose(pm.corr(), np.corrcoef(T.T) * 0 + ref / scale, rtol=1e-11, atol=1e-13)
    assert not pm.constant().any()


def test_deviation_vector_is_theta_minus_the_updated_mean():
    T = _thetas()
    pm = PP.ParamMoments(list('abcd'))
    W = 0
    C = np.zeros((4, 4))
    m = np.zeros(4)
    for n, (t, w) in enumerate(zip(T, WEIGHTS)):
        before = pm.mean()
        e = pm.update(t, w)
        W += w
        assert np.array_equal(e, t - pm.mean())                 # the definition: the mean AFTER the member
        if n == 0:
            assert np.array_equal(pm.mean(), t) and not e.any()  # the first member is the mean, exactly
        else:
            assert np.array_equal(pm.mean(), before + (t - before) * float(w) / float(W))
            C = C + np.outer(float(w) * (t - before), e)
        m = pm.mean()
        assert np.array_equal(pm.C, C)
    assert np.array_equal(m, pm.m)


def test_merge_equals_one_pass():
    T = _thetas(8)
    names = list('abcd')
    all_ = _fill(names, T, WEIGHTS)
    a, b = _fill(names, T[:3], WEIGHTS[:3]), _fill(names, T[3:], WEIGHTS[3:])
    ma, mb = a.mean(), b.mean()
    dtheta = a.merge(b)
    assert np.array_equal(dtheta, mb - ma)
    assert a.W == all_.W and a.members == all_.members
    np.testing.assert_allclose(a.mean(), all_.mean(), rtol=1e-14)
    sd = np.sqrt(np.diag(all_.cov()))
    assert np.all(np.abs(a.cov() - all_.cov()) <= 1e-12 * np.outer(sd, sd))
    # into an empty one: a copy; from an empty one: nothing
    e = PP.ParamMoments(names)
    e.merge(all_)
    assert np.array_equal(e.C, all_.C) and np.array_equal(e.m, all_.m) and e.W == all_.W
    keep = e.C.copy()
    assert not e.merge(PP.ParamMoments(names)).any() and np.array_equal(e.C, keep)
    with pytest.raises(ValueError, match='different scalars'):
        e.merge(PP.ParamMoments(list('abc')))


def test_factor_of_a_rank_deficient_set():
    T = _thetas(8, 3)
    T = np.column_stack([T, T[:, 1], np.full(len(T), 0.25)])        # a duplicated and a constant column
    pm = _fill(list('abcde'), T, WEIGHTS)
    assert pm.constant().tolist() == [False, False, False, False, True]
    assert pm.inv_sd()[4] == 0.0 and pm.cov()[4, 4] == 0.0 and not pm.corr()[4].any()
    F, rank, lam = pm.factor()
    assert rank == 3 and F.shape == (5, 3) and lam.size == 4
    assert not F[4].any()                                            # the constant scalar's row
    assert np.all(np.diff(lam) <= 0) and abs(lam[3]) < 1e-12 * lam[0]    # the dropped one is reported
    S = pm.cov()
    G = F @ F.T
    assert np.abs(G @ S @ G - G).max() <= 1e-10 * np.abs(G).max()
    assert np.abs(S @ G @ S - S).max() <= 1e-10 * np.abs(S).max()
    np.testing.assert_allclose(G[:4, :4], np.linalg.pinv(S[:4, :4], rcond=1e-12), rtol=1e-7,
                               atol=1e-10 * np.abs(G).max())
    # everything constant: rank 0, and finalize has nothing to explain
    c = _fill(['a', 'b'], np.ones((4, 2)), [1, 2, 1, 1])
    F, rank, lam = c.factor()
    assert rank == 0 and F.shape == (2, 0) and c.constant().all() and not c.C.any()
    with pytest.raises(ValueError, match='no sensitivity parameter varies'):
        PP.finalize_factor(c)


def test_finalize_needs_rank_plus_two_members():
    T = _thetas(8, 3)
    for n in (1, 2, 3, 4):
        pm = _fill(list('abc'), T[:n], WEIGHTS[:n])
        with pytest.raises(ValueError, match='members'):
            PP.finalize_factor(pm)                                    # rank = min(n - 1, 3): n < rank + 2
    pm = _fill(list('abc'), T[:5], WEIGHTS[:5])
    F, rank, lam, isd = PP.finalize_factor(pm)
    assert rank == 3 and F.flags['C_CONTIGUOUS'] and F.dtype == np.float64 and isd.shape == (3,)
    # a heavy weight is still one member
    two = _fill(list('abc'), T[:2], [40, 60])
    with pytest.raises(ValueError, match='2 members for 1 independent'):
        PP.finalize_factor(two)
    with pytest.raises(ValueError, match='nothing accumulated'):
        PP.finalize_factor(PP.ParamMoments(['a']))


def test_name_and_limit_checks():
    assert PP.check_sens_params(None) == NAMES and PP.check_sens_params(True) == NAMES and len(NAMES) == 15
    assert PP.check_sens_params(['mu_r', 'sig_x']) == ['mu_r', 'sig_x']
    assert PP.check_sens_params('lam') == ['lam']
    with pytest.raises(ValueError, match="unknown sensitivity parameters \\['nope'\\]"):
        PP.check_sens_params(['sig_x', 'nope'])
    with pytest.raises(ValueError, match='unknown'):
        PP.check_sens_params(['xi'])                                  # a nuisance parameter: not in the fields
    with pytest.raises(ValueError, match='0 sensitivity parameters'):
        PP.check_sens_params([])
    with pytest.raises(ValueError, match='listed twice'):
        PP.check_sens_params(['sig_x', 'sig_x'])
    with pytest.raises(ValueError, match='list of names'):
        PP.check_sens_params(3)
    with pytest.raises(ValueError, match='17 scalars'):
        PP.ParamMoments(['p%d' % i for i in range(17)])
    with pytest.raises(ValueError, match='0 scalars'):
        PP.ParamMoments([])
    pm = PP.ParamMoments(['a', 'b'])
    with pytest.raises(ValueError, match='3 scalars given'):
        pm.update([1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match='finite'):
        pm.update([1.0, np.nan])
    for w in (0, -1, 1.5):
        with pytest.raises(ValueError, match='positive integer'):
            pm.update([1.0, 2.0], w)
    pm.update([1.0, 2.0], 2 ** 32 - 1)
    with pytest.raises(ValueError, match='2\\^32'):
        pm.update([1.0, 2.0], 1)
    assert pm.W == 2 ** 32 - 1 and pm.members == 1                    # a refused update changes nothing
    with pytest.raises(ValueError, match='nothing accumulated'):
        PP.ParamMoments(['a']).cov()


def _plume(n, shape=(65, 63), seed=1):
    """synthetic plume fields: a Gaussian bump whose place, width and height move with the scalars, zero
    outside a threshold -- so most cells are 0 in every member and some only in a few"""
    rng = np.random.default_rng(seed)
    T = rng.normal(size=(n, 3)) * [1.5, 0.3, 0.1] + [30.0, 2.5, 1.0]
    r, c = np.mgrid[:shape[0], :shape[1]]
    X = []
    for cx, sg, amp in T:
        f = 1e3 * amp * np.exp(-((r - 30.0) ** 2 + (c - cx) ** 2) / (2 * sg ** 2))
        X.append(np.where(f >= 1.0, f, 0.0))
    return np.array(X), T


def test_replay_matches_a_two_pass_covariance():
    X, T = _plume(8)
    pm = PP.ParamMoments(['cx', 'sg', 'amp'])
    st = sens_ref.new_state(X[0].shape, 3)
    for x, t, w in zip(X, T, WEIGHTS):
        sens_ref.add(st, x, pm.update(t, w), w)
    W = float(sum(WEIGHTS))
    assert st['W'] == W
    mean, var, cov, tcov = sens_ref.two_pass(X, T, WEIGHTS)
    scale = np.abs(mean).max()
    np.testing.assert_allclose(st['mean'], mean, rtol=1e-12, atol=1e-15 * scale)
    np.testing.assert_allclose(st['M2'] / W, var, rtol=1e-12, atol=1e-15 * scale ** 2)
    sd = np.sqrt(np.diag(tcov))
    for i in range(3):
        np.testing.assert_allclose(st['C'][i] / W, cov[i], rtol=1e-12, atol=1e-15 * scale * sd[i])
    np.testing.assert_allclose(pm.cov(), tcov, rtol=1e-12, atol=1e-15 * sd.max() ** 2)
    dead = ~(X != 0).any(axis=0)
    assert dead.sum() > dead.size // 2                                 # most of the domain
    assert not st['mean'][dead].any() and not st['C'][:, dead].any() and not st['M2'][dead].any()
    # the finalize of the replay: a share in [0, 1], the index of the largest |correlation|, -1 where nothing varies
    F, rank, _lam, isd = PP.finalize_factor(pm)
    expl, dom = sens_ref.finalize(st['C'] / W, st['M2'] / W, F, isd)
    assert rank == 3 and expl.min() >= 0.0 and expl.max() <= 1.0 + 1e-9 and expl.max() > 0.5
    assert np.array_equal(dom == -1, st['M2'] == 0.0) and not expl[st['M2'] == 0.0].any()
    corr = np.array([cov[i] / np.sqrt(np.where(var > 0, var, 1.0) * tcov[i, i]) for i in range(3)])
    clear = (var > 0) & (np.sort(np.abs(corr), axis=0)[-1] - np.sort(np.abs(corr), axis=0)[-2] > 1e-6)
    assert clear.sum() > 20 and np.array_equal(dom[clear], np.argmax(np.abs(corr), axis=0)[clear])
    # explained against the weighted least-squares fit of every cell on the scalars
    w = np.asarray(WEIGHTS, dtype=float)
    A = np.column_stack([np.ones(len(T)), T]) * np.sqrt(w)[:, None]
    Y = (X.reshape(len(X), -1) * np.sqrt(w)[:, None])
    res = Y - A @ np.linalg.lstsq(A, Y, rcond=None)[0]
    r2 = 1.0 - (res ** 2).sum(0) / W / np.where(var.ravel() > 0, var.ravel(), 1.0)
    live = var.ravel() > 1e-6 * var.max()
    np.testing.assert_allclose(expl.ravel()[live], r2[live], atol=1e-8)


def test_a_bad_name_fails_before_any_evaluation():
    tr = np.array([[m[2] for m in mcmc.MODEL_BLOCK]] * 3)
    calls = []

    def evaluate(theta):
        calls.append(theta)
        return None
    for bad in (['nope'], ['sig_x', 'xi'], [], ['mu_r', 'mu_r']):
        with pytest.raises(ValueError, match='sensitivity'):
            PP.posterior_predictive(None, (tr, NAMES), evaluate=evaluate, sensitivity=bad)
    assert calls == []
    res = PP.posterior_predictive(None, (tr, NAMES), evaluate=evaluate, sensitivity=['mu_r'])
    assert len(calls) == 1 and res.sensitivity is None and res.failed == 1        # no device: no maps


def test_signed_maps_keep_negative_entries(tmp_path):
    from scipy import sparse
    m = np.array([[0.5, -0.25, 0.0], [1e-9, -1e-9, -1.0]])
    PP.save_maps(str(tmp_path / 's'), [(3, [('_corr_x', m)])], {'3_dom': np.array([[0, -1]], dtype=np.int8)},
                 signed=True)
    PP.save_maps(str(tmp_path / 'u'), [(3, [('_corr_x', m)])])
    with np.load(tmp_path / 's.npz') as f:
        got = sparse.csr_matrix((f['3_corr_x_data'], f['3_corr_x_ind'], f['3_corr_x_indptr']), shape=m.shape)
        assert np.array_equal(got.toarray(), np.where(np.abs(m) >= 1e-8, m, 0.0))
        assert f['3_dom'].dtype == np.int8 and list(f['days']) == [3]
    with np.load(tmp_path / 'u.npz') as f:                              # the unsigned writer is as it was
        got = sparse.csr_matrix((f['3_corr_x_data'], f['3_corr_x_ind'], f['3_corr_x_indptr']), shape=m.shape)
        assert np.array_equal(got.toarray(), np.where(m >= 1e-8, m, 0.0))
