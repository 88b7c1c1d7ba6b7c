"""Host-side tests of the ensemble modes (predictive.mode_decomposition, separated, score_drivers, check_modes and
the driver's request check) against the numpy restatement modes_ref, which goes through the SVD of the weighted
anomalies where the package goes through the eigen-decomposition of the table.

Tolerances.  eps = 2^-53.  numpy.linalg.eigh returns the exact eigenvalues of B + E with |E|_2 <= c M eps |B|_2 and
the SVD the exact singular values of Y + F with |F|_2 <= c M eps |Y|_2 (LAPACK's backward errors, c a small constant;
squared, the latter moves lambda by 2 c M eps lambda_1); the table enters rounded once per entry and B costs three more
roundings per entry, at most 4 M eps |B|_2 in norm.  With c <= 4 and |B|_2 <= trace B all of it stays below
  dB = 16 M eps trace B,
the eigenvalue tolerance.  An eigenvector of a symmetric matrix moves by at most 2 |dB| / gap (Davis & Kahan 1970),
gap the distance of lambda_k to the nearest other eigenvalue; the unit pattern is e_k = Y^T u_k / sqrt(lambda_k) with
|Y|_2 = sqrt(lambda_1), so it moves by sqrt(lambda_1 / lambda_k) 2 dB / gap, plus dB / (2 lambda_k) from lambda_k
itself, plus the rounding of the M-term sum that forms it, M eps |c|_2 |A|_F <= M eps sqrt(W trace B / lambda_k).  A
score z_mk = u_mk sqrt(W / w_m) moves by sqrt(W) 2 dB / gap at most."""
import os
import types

import numpy as np
import pytest

import modes_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53


def _ensemble(seed, M, P, spectrum=None):
    """(A [M, P] weighted-centred anomalies, integer weights); spectrum: the eigenvalues of B, descending (at most
    M - 1: centring leaves that many)"""
    rng = np.random.default_rng(seed)
    w = rng.integers(1, 6, M)
    A = rng.standard_normal((M, P)) * rng.uniform(0.5, 3.0, (M, 1))
    A = A - (w[:, None] * A).sum(0) / w.sum()
    if spectrum is not None:
        s = np.sqrt(w / w.sum())
        U, _s, Vt = np.linalg.svd(s[:, None] * A, full_matrices=False)
        S = np.zeros(M)
        S[:len(spectrum)] = np.sqrt(spectrum)
        A = (U * S) @ Vt / s[:, None]
    return A, w


def _tolerances(ref, M, W):
    lam = ref['spectrum']
    dB = 16 * M * EPS * ref['total_variance']
    out = []
    for k in range(len(ref['eigenvalues'])):
        gap = min(abs(lam[k] - lam[j]) for j in range(len(lam)) if j != k)
        vec = 2 * dB / gap
        pat = (np.sqrt(lam[0] / lam[k]) * vec + dB / (2 * lam[k])
               + M * EPS * np.sqrt(W * ref['total_variance'] / lam[k]))
        out.append((vec, pat))
    return dB, out


def _compare(A, w, K):
    from parasitoids_amd.predictive import mode_decomposition
    M = len(w)
    G = R.table(A).astype(np.float64)
    dec = mode_decomposition(G, w, K)
    ref = R.decomposition(A, w, K)
    dB, tol = _tolerances(ref, M, float(w.sum()))
    assert dec['count'] == K
    assert np.all(np.abs(dec['eigenvalues'] - ref['eigenvalues']) <= dB), (dec['eigenvalues'], ref['eigenvalues'])
    assert abs(dec['total_variance'] - ref['total_variance']) <= dB
    assert np.all(np.abs(dec['explained'] - ref['explained']) <= 2 * dB / ref['total_variance'])
    pat = dec['coef'] @ A
    for k in range(K):
        vec, ptol = tol[k]
        assert np.linalg.norm(dec['vectors'][:, k] - ref['vectors'][:, k]) <= vec, (k, vec)
        assert np.linalg.norm(pat[k] - ref['patterns'][k]) <= ptol, (k, ptol)
        assert np.abs(dec['scores'][:, k] - ref['scores'][:, k]).max() <= np.sqrt(w.sum()) * vec
        assert abs(np.linalg.norm(pat[k]) - 1.0) <= 2 * ptol
    # the standardised scores: weighted mean 0 and variance 1
    z = dec['scores']
    assert np.abs((w[:, None] * z).sum(0) / w.sum()).max() <= 64 * M * EPS * np.abs(z).max()
    assert np.abs((w[:, None] * z * z).sum(0) / w.sum() - 1.0).max() <= 64 * M * EPS
    return dec, ref, tol


@pytest.mark.parametrize('seed,M,P', [(1, 4, 30), (2, 7, 50), (3, 12, 200), (4, 9, 17)])
def test_decomposition_against_the_svd(seed, M, P):
    spectrum = (3.0 * 0.55 ** np.arange(M - 1))          # relative gaps of 0.45: well separated
    A, w = _ensemble(seed, M, P, spectrum)
    assert len(set(w.tolist())) > 1
    _compare(A, w, min(M - 1, 8))


def test_patterns_at_a_relative_eigengap_of_two_thousandths():
    M, P = 8, 120
    spectrum = np.array([4.0, 4.0 * (1 - 2e-3), 1.0, 0.5, 0.1, 0.01, 0.001])
    A, w = _ensemble(11, M, P, spectrum)
    dec, ref, tol = _compare(A, w, 5)
    assert tol[0][0] < 1e-9                # the tolerance is still a statement
    assert np.abs(dec['eigenvalues'] - spectrum[:5]).max() <= 16 * M * EPS * spectrum.sum() * 2


def test_splitting_a_weight_changes_nothing():
    from parasitoids_amd.predictive import mode_decomposition
    A, w = _ensemble(5, 6, 80, 2.0 * 0.5 ** np.arange(5))
    w = w.copy()
    w[2] = 3
    A = A - (w[:, None] * A).sum(0) / w.sum()
    A2 = np.vstack([A[:3], A[2:3], A[2:3], A[3:]])
    w2 = np.concatenate([w[:3], [1, 1], w[3:]])
    w2[2] = 1
    K = 4
    one = mode_decomposition(R.table(A).astype(np.float64), w, K)
    two = mode_decomposition(R.table(A2).astype(np.float64), w2, K)
    ref = R.decomposition(A, w, K)
    dB, tol = _tolerances(ref, len(w2), float(w.sum()))
    assert np.all(np.abs(one['eigenvalues'] - two['eigenvalues']) <= 2 * dB)
    p1, p2 = one['coef'] @ A, two['coef'] @ A2
    for k in range(K):
        vec, ptol = tol[k]
        # the copies share the entry of largest magnitude or not: compare up to the sign the rule gave
        s = 1.0 if np.dot(p1[k], p2[k]) > 0 else -1.0
        assert np.linalg.norm(p1[k] - s * p2[k]) <= 2 * ptol, k
        z1, z2 = one['scores'][:, k], s * two['scores'][:, k]
        ztol = 2 * np.sqrt(w.sum()) * vec
        assert np.abs(z2[2:5] - z1[2]).max() <= ztol and np.abs(z2[:2] - z1[:2]).max() <= ztol
        assert np.abs(z2[5:] - z1[3:]).max() <= ztol


def test_the_sign_rule_and_its_tie():
    from parasitoids_amd.predictive import mode_decomposition
    # two members of equal weight: u = (1, -1) / sqrt(2), both entries of the same magnitude: the first is positive
    for G in ([[1.0, -1.0], [-1.0, 1.0]], [[4.0, -4.0], [-4.0, 4.0]]):
        dec = mode_decomposition(np.array(G), [1, 1], 1)
        u = dec['vectors'][:, 0]
        assert abs(u[0]) == abs(u[1]) and u[0] > 0 > u[1]
    # the entry of largest magnitude decides, wherever it is
    A = np.array([[1.0, 0.0], [2.0, 0.0], [-3.0, 0.0]])
    dec = mode_decomposition(A @ A.T, [1, 1, 1], 1)
    assert dec['vectors'][2, 0] > 0 and dec['vectors'][0, 0] < 0
    assert np.array_equal(R.sign_rule(np.array([0.5, -0.5])), [0.5, -0.5])
    assert np.array_equal(R.sign_rule(np.array([-0.5, 0.5])), [0.5, -0.5])
    assert np.array_equal(R.sign_rule(np.array([0.1, -0.9, 0.9])), [-0.1, 0.9, -0.9])


def test_a_rank_deficient_table_shrinks_the_count():
    from parasitoids_amd.predictive import mode_decomposition
    rng = np.random.default_rng(3)
    x, y = rng.standard_normal(40), rng.standard_normal(40)
    X = np.array([x, x, y])                       # two identical members
    w = np.array([2, 1, 3])
    A = X - (w[:, None] * X).sum(0) / w.sum()
    dec = mode_decomposition(A @ A.T, w, 3)
    assert dec['count'] == 1 and len(dec['eigenvalues']) == 1 and dec['coef'].shape == (1, 3)
    assert dec['scores'].shape == (3, 1) and np.isfinite(dec['coef']).all()
    assert abs(dec['explained'][0] - 1.0) <= 16 * 3 * EPS * 4
    # no variance at all: nothing kept, nothing divided
    dec = mode_decomposition(np.zeros((3, 3)), w, 2)
    assert dec['count'] == 0 and dec['coef'].shape == (0, 3) and dec['total_variance'] == 0.0
    for bad in (0, 9, True):
        with pytest.raises(ValueError):
            mode_decomposition(A @ A.T, w, bad)
    with pytest.raises(ValueError):
        mode_decomposition(A @ A.T, [1, 0, 1], 1)
    with pytest.raises(ValueError):
        mode_decomposition(np.zeros((2, 2)), w, 1)


def test_separated_is_norths_rule():
    from parasitoids_amd.predictive import effective_members, separated
    w = [1, 3, 1, 2, 1]
    assert effective_members(w) == R.n_eff(w) == 64.0 / 16.0
    lam = [10.0, 9.0, 2.0, 0.5]
    # n_eff = 4: the error is lambda / sqrt(2); 10 and 9 are a plane, 2 stands clear of 0.5 (1.5 > 1.41), 0.5 of 2
    assert separated(lam, w).tolist() == R.separated(lam, w) == [False, False, True, True]
    big = [1] * 200
    # n_eff = 200: the error is lambda / 10; a mode is judged by its own error: 1 is not > 1.0, but it is > 0.9
    assert separated(lam, big).tolist() == R.separated(lam, big) == [False, True, True, True]
    assert separated([10.0, 9.5, 2.0, 0.5], big).tolist() == [False, False, True, True]
    assert separated([10.0, 5.0, 2.0], big).tolist() == [True, True, True]
    assert separated([3.0], w).tolist() == [True]
    rng = np.random.default_rng(0)
    for _ in range(20):
        lam = np.sort(rng.random(6))[::-1]
        ww = rng.integers(1, 5, 30)
        assert separated(lam, ww).tolist() == R.separated(lam, ww)


def test_score_drivers_is_the_weighted_correlation():
    from parasitoids_amd.predictive import score_drivers
    rng = np.random.default_rng(4)
    M = 12
    w = rng.integers(1, 4, M)
    th = rng.standard_normal((M, 4))
    th[:, 2] = 171.82                              # a parameter the chain never moved
    z = np.column_stack([3.0 * th[:, 0] - 1.0, rng.standard_normal(M), -th[:, 3] + 0.1 * rng.standard_normal(M)])
    names = ['a', 'b', 'c', 'd']
    got = score_drivers(z, th, w, names)
    ref = R.score_drivers(z, th, w)
    assert got['names'] == names and got['corr'].shape == (3, 4)
    assert np.abs(got['corr'] - ref).max() <= 64 * M * EPS
    assert abs(got['corr'][0, 0] - 1.0) <= 64 * M * EPS and np.all(got['corr'][:, 2] == 0.0)
    assert got['strongest'][0] == 'a' and got['strongest'][2] == 'd' and got['corr'][2, 3] < -0.9
    assert score_drivers(np.zeros((M, 1)), th, w, names)['strongest'] == [None]
    with pytest.raises(ValueError):
        score_drivers(z, th[:, :3], w, names)


def test_check_modes():
    from parasitoids_amd.predictive import check_modes
    assert check_modes(True, 6) == {'days': 'all', 'count': 4, 'transform': 'sqrt'}
    assert check_modes(dict(days=[1, 5], count=3, transform='raw'), 6) == {'days': [1, 5], 'count': 3,
                                                                           'transform': 'raw'}
    assert check_modes(dict(days='all', count=8), [0, 2, 4])['days'] == 'all'
    assert check_modes(dict(days=[2, 4]), [0, 2, 4])['days'] == [2, 4]
    assert check_modes(dict(days=list(range(8))), 30)['days'] == list(range(8))
    bad = [False, None, 4, [1, 2], dict(day=[1]), dict(count=0), dict(count=9), dict(count=2.5), dict(count=True),
           dict(transform='log'), dict(days=[6]), dict(days=[-1]), dict(days=[]), dict(days=[3, 1]), dict(days=[1, 1]),
           dict(days='some'), dict(days=5), dict(days=['a'])]
    for arg in bad:
        with pytest.raises(ValueError):
            check_modes(arg, 6)
    with pytest.raises(ValueError, match='at most 8'):
        check_modes(True, 9)                       # 'all' over more than 8 days
    with pytest.raises(ValueError, match='8 days'):
        check_modes(dict(days=list(range(9))), 30)
    with pytest.raises(ValueError, match='not among'):
        check_modes(dict(days=[1]), [0, 2, 4])


def test_posterior_predictive_refuses_before_any_evaluation():
    from parasitoids_amd import predictive as PR
    calls = []

    def evaluate(theta):
        calls.append(theta)
        return None
    chain = (np.zeros((3, len(PR.model_names()))), PR.model_names())
    with pytest.raises(ValueError, match='modes= needs the device'):
        PR.posterior_predictive(None, chain, evaluate=evaluate, modes=True)
    pm = types.SimpleNamespace(days=list(range(6)), rad_dist=10000.0, rad_res=400, solver=None)
    for arg, match in ((dict(count=9), 'count'), (dict(days=[6]), 'not among'), (dict(transform='log'), 'transform'),
                       (dict(days=list(range(9))), '8 days'), (5, 'modes must be')):
        with pytest.raises(ValueError, match=match):
            PR.posterior_predictive(pm, chain, modes=arg)
    with pytest.raises(ValueError, match='at most 8'):
        PR.posterior_predictive(types.SimpleNamespace(days=list(range(12)), rad_dist=1e4, rad_res=400), chain,
                                modes=True)
    with pytest.raises(ValueError, match='not among'):      # 'all' means the summary's days; a listed day the model's
        PR.posterior_predictive(pm, chain, days=[0, 2], modes=dict(days=[7]))
    assert not calls


def test_without_modes_nothing_is_built():
    from parasitoids_amd import predictive as PR
    for kind in ('days', 'sites'):
        assert PR.FEED_ORDER[kind][-1] == 'modes'
    assert 'modes' not in PR.FEED_ORDER['projection'] and 'modes' not in PR.FEED_ORDER['compare']
    assert 'modes' in PR.ACCUMULATORS and 'modes' in PR.BUILD
    fs = PR._FieldSet().fed_from('days', object(), owns=False)
    assert PR.BUILD['modes'](fs, types.SimpleNamespace(md_plan=None)) is None and fs.modes is None
    chain = (np.zeros((3, len(PR.model_names()))), PR.model_names())
    res = PR.posterior_predictive(None, chain, evaluate=lambda theta: None)
    assert res.modes is None
    assert PR.EnsembleModes._prefix == 'ps_modes' and PR.MODE_TRANSFORMS == {'raw': 0, 'sqrt': 1}
    src = open(os.path.join(ROOT, 'scripts', 'run_predictive.py')).read()
    for flag in ('--modes', '--modes-days', '--modes-transform', 'modes_table_ms', 'modes_add_ms_per_member'):
        assert flag in src


def test_the_driver_names_the_memory_it_lacks():
    from parasitoids_amd import _lib as L
    from parasitoids_amd import predictive as PR

    class Full():
        modes = types.SimpleNamespace(days=[1, 2], pitch=641664)

        def reserve(self, n):
            raise L.HipError(L.PS_ERR_OOM, "modes_reserve: the members' fields need 10.5 GB, 1 GB free")
    with pytest.raises(ValueError, match=r'1024 members x 2 days x 641664 cells x 8 B = 10\.5 GB'):
        PR._reserve_modes(Full(), 1024)

    class Broken(Full):
        def reserve(self, n):
            raise L.HipError(L.PS_ERR_HIP, 'something else')
    with pytest.raises(L.HipError):
        PR._reserve_modes(Broken(), 4)
