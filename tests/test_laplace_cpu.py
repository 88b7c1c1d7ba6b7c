"""CPU tests of parasitoids_amd/laplace.py (MAP fit and normal approximation, Bayes_MAP.py): the
finite-difference Hessian, the composed log posterior, evaluation counts, boundary steps, the
non-positive-definite path, the MAP search, reproducibility, chain starts, the result files and the
shared map writer.  No device: expected observations come from `evaluate=`."""
import types
import zipfile

import numpy as np
import pytest

from parasitoids_amd import laplace as LA
from parasitoids_amd import mcmc
from parasitoids_amd import predictive as PP


def _locinfo(g, seed=4):
    rng = np.random.default_rng(seed)
    li = types.SimpleNamespace()
    li.sent_ids = ['A', 'B', 'C']
    li.field_sizes = {k: len(g['field_' + k]) for k in li.sent_ids}
    li.release_collection = [np.full(g['rel0'].shape[0], 1.0), np.full(g['rel1'].shape[0], 0.5)]
    li.grid_samples = np.full(g['grid'].shape, 2.0)
    cell_area = (10000.0 / 128) ** 2
    sp = mcmc.initial_sent_obs_probs(li, cell_area)
    li.release_emerg = [rng.poisson(0.75 * g['rel%d' % i] * (li.release_collection[i] * 0.05)[:, None]) for i in range(2)]
    li.sentinel_emerg = [rng.poisson(0.75 * g['sen%d' % i] * sp[:, None]) for i in range(2)]
    li.grid_obs = rng.poisson(0.005 * li.grid_samples * g['grid'])
    return li, cell_area


def _evaluator(g, calls=None, reject=None):
    """expected observations = the fixture's arrays scaled by a smooth positive function of theta"""
    base = ([g['rel0'], g['rel1']], [g['sen0'], g['sen1']], g['grid'])
    t0 = np.array([m[2] for m in mcmc.MODEL_BLOCK])
    w = np.linspace(0.5, 1.5, t0.size)

    def evaluate(theta):
        if calls is not None:
            calls.append(np.array(theta))
        if reject is not None and reject(theta):
            return None
        f = float(np.exp(0.3 * np.tanh((w * (theta / t0 - 1.0)).sum())))
        return ([f * r for r in base[0]], [f * s for s in base[1]], f * base[2])
    return evaluate


@pytest.fixture
def site(golden):
    g = golden('g9_bayes_funcs')
    li, cell_area = _locinfo(g)
    return g, li, cell_area


# ---------------------------------------------------------------- 1. the Hessian utility
def test_hessian_exact_for_a_quadratic_and_second_order_otherwise():
    rng = np.random.default_rng(1)
    d = 6
    A = rng.normal(size=(d, d))
    Q = -(A @ A.T + d * np.eye(d))
    b = rng.normal(size=d)
    x = rng.normal(size=d)
    h = np.full(d, 0.1)
    f = lambda y: 0.5 * y @ Q @ y + b @ y + 3.0
    H, g, f0 = LA.hessian(f, x, h)
    np.testing.assert_allclose(H, Q, rtol=0, atol=1e-10 * np.abs(Q).max())
    np.testing.assert_allclose(g, Q @ x + b, rtol=0, atol=1e-11 * np.abs(Q).max())
    assert f0 == f(x)
    assert np.array_equal(H, H.T)
    # smooth, not quadratic: the error falls as h^2
    c = rng.normal(size=d)
    f2 = lambda y: float(np.exp(c @ y * 0.3)) + np.sin(y).sum()
    e = np.exp(0.3 * c @ x)
    exact = 0.09 * e * np.outer(c, c) - np.diag(np.sin(x))
    errs = [np.abs(LA.hessian(f2, x, np.full(d, s))[0] - exact).max() for s in (0.04, 0.02)]
    assert errs[1] < errs[0] / 3.0 and errs[1] < 1e-3
    # a zero step holds the row and column
    H0 = LA.hessian(f, x, np.array([0.1, 0.0, 0.1, 0.1, 0.1, 0.1]))[0]
    assert not H0[1].any() and not H0[:, 1].any()


# ---------------------------------------------------------------- 2./3. composed posterior, counts
def test_normal_approx_equals_the_utility_on_the_composed_posterior(site):
    g, li, cell_area = site
    ev = _evaluator(g)
    res = LA.normal_approx(None, li, cell_area, evaluate=ev)
    areas = mcmc.field_areas(li, cell_area)
    nm = len(LA.FREE_MODEL)

    def f(x):
        theta = np.empty(15)
        theta[LA.FREE_MODEL] = x[:nm]
        theta[13] = 30.0
        nuis, A, sp = x[nm:nm + 3], x[nm + 3], x[nm + 4:]
        st = mcmc.lik_stats(ev(theta), li)
        return mcmc.log_prior(theta, nuis, A, sp, areas) + sum(mcmc.loglik_parts_stats(st, nuis, sp))
    H, gr, f0 = LA.hessian(f, res.mu, res.steps)
    assert np.array_equal(H, res.H) and np.array_equal(gr, res.grad) and f0 == res.logp
    assert res.names == LA.free_names(li) and res.held == []
    eps = np.array([LA.PRIOR_EPS[i][1] for i in LA.FREE_MODEL])
    assert np.array_equal(res.steps[:nm], eps)        # nothing near a bound at the start
    assert res.spread is None and res.C.shape == (len(res.names),) * 2


def test_hessian_costs_exactly_393_model_evaluations(site):
    g, li, cell_area = site
    calls = []
    res = LA.normal_approx(None, li, cell_area, evaluate=_evaluator(g, calls))
    m = 14
    assert len(calls) == res.evaluations == 1 + 2 * m + 2 * m * (m - 1) == 393
    assert len({c.tobytes() for c in calls}) == 393           # each model point once
    assert all(c[13] == 30.0 for c in calls)                    # n_periods held
    # the stencil has far more points: those that move only nuisance parameters cost nothing
    d = len(res.names)
    assert 1 + 2 * d + 2 * d * (d - 1) > 393


# ---------------------------------------------------------------- 4. boundaries
def test_steps_shrink_near_a_bound_and_hold_on_it(site):
    g, li, cell_area = site
    names = [m[0] for m in mcmc.MODEL_BLOCK]
    theta = np.array([m[2] for m in mcmc.MODEL_BLOCK])
    theta[names.index('f_a1')] = 9.0 - 0.03          # TruncatedNormal upper bound 9, eps 0.1
    theta[names.index('lam')] = 1.0 - 1e-7           # Beta, eps 0.01: would shrink below 1e-3 eps -> held
    calls = []
    res = LA.normal_approx(None, li, cell_area, at=theta, evaluate=_evaluator(g, calls))
    i_f = res.names.index('f_a1')
    i_l = res.names.index('lam')
    assert res.steps[i_f] == pytest.approx(0.015)
    assert res.steps[i_l] == 0.0 and res.held == ['lam']
    assert not res.C[i_l].any() and not res.H[i_l].any()
    m = 13
    assert res.evaluations == 1 + 2 * m + 2 * m * (m - 1)
    assert all(c[names.index('f_a1')] <= 9.0 for c in calls)
    h = LA.stencil_steps([0.0, 0.5, 5.0], [0.0, 0.0, 0.0], [1.0, 1.0, np.inf], [0.1, 0.6, 1.0])
    assert h[0] == 0.0 and h[1] == 0.25 and h[2] == 1.0


# ---------------------------------------------------------------- 5. not positive definite
def test_non_positive_definite_is_reported_not_fixed():
    H = np.diag([-2.0, 1.0, -3.0])
    C, pd, w = LA._covariance(H, np.ones(3))
    assert not pd and w.min() < 0
    np.testing.assert_allclose(np.sort(w), [-1.0, 2.0, 3.0])
    np.testing.assert_allclose(C, np.diag([0.5, 0.0, 1.0 / 3.0]))
    F = LA.model_factor(C, 3, pd)
    np.testing.assert_allclose(F @ F.T, C, atol=1e-15)
    C2, pd2, _ = LA._covariance(np.diag([-2.0, -4.0]), np.ones(2))
    assert pd2 and np.allclose(C2, np.diag([0.5, 0.25]))


def test_normal_approx_away_from_the_mode_can_be_indefinite(site):
    g, li, cell_area = site
    ev = _evaluator(g)
    li2 = types.SimpleNamespace(**vars(li))
    li2.grid_obs = li.grid_obs * 0           # a likelihood whose curvature changes sign in theta
    res = LA.normal_approx(None, li2, cell_area, evaluate=ev)
    assert res.pd == bool(np.all(res.eigenvalues > 0))
    if not res.pd:
        F = res.F
        assert np.all(np.isfinite(F))


# ---------------------------------------------------------------- 6./7. the MAP search
def test_find_map_improves_and_is_a_local_maximum(site):
    g, li, cell_area = site
    r = LA.find_map(None, li, cell_area, evaluate=_evaluator(g), maxeval=600)
    assert r.logp >= r.logp_start and r.logp > r.logp_start + 1.0
    post = LA.Posterior(None, li, cell_area, 30.0, evaluate=_evaluator(g))
    assert post.logp(r.x) == pytest.approx(r.logp, abs=1e-9 * abs(r.logp))
    h = LA.stencil_steps(r.x, post.lo, post.hi, post.eps)
    tol = 1e-3
    for i in range(len(r.x)):
        for s in (1, -1):
            if h[i]:
                assert post.logp(LA.axis_point(r.x, h, i, s)) <= r.logp + tol, (r.names[i], s)
    assert r.evaluations <= 600 and r.failed == 0 and r.k == len(LA.free_names(li))


def test_two_runs_give_identical_bits(site):
    g, li, cell_area = site
    a = LA.find_map(None, li, cell_area, evaluate=_evaluator(g), maxeval=120)
    b = LA.find_map(None, li, cell_area, evaluate=_evaluator(g), maxeval=120)
    assert np.array_equal(a.x, b.x) and a.logp == b.logp and a.evaluations == b.evaluations
    na = LA.normal_approx(None, li, cell_area, at=a, evaluate=_evaluator(g))
    nb = LA.normal_approx(None, li, cell_area, at=b, evaluate=_evaluator(g))
    assert np.array_equal(na.H, nb.H) and np.array_equal(na.C, nb.C) and np.array_equal(na.F, nb.F)


def test_failed_evaluations_count_and_score_minus_infinity(site):
    g, li, cell_area = site
    reject = lambda th: th[0] > 1.02          # g_aw above 1.02 is "rejected by the model"
    r = LA.find_map(None, li, cell_area, evaluate=_evaluator(g, reject=reject), maxeval=150)
    assert r.failed > 0 and r.theta[0] <= 1.02 and np.isfinite(r.logp)
    with pytest.raises(ValueError):
        LA.normal_approx(None, li, cell_area, at=np.r_[1.0 + 0.02, r.theta[1:]],
                         evaluate=_evaluator(g, reject=reject))


# ---------------------------------------------------------------- 8. chain starts
def test_start_from_chain_picks_the_maximum_row(site, tmp_path):
    g, li, cell_area = site
    names = ([m[0] for m in mcmc.MODEL_BLOCK] + [m[0] for m in mcmc.NUISANCE] + ['A_collected']
             + ['sent_obs_probs_%s' % k for k in li.sent_ids])
    rng = np.random.default_rng(5)
    tr1, tr2 = rng.random((7, len(names))), rng.random((5, len(names)))
    lp1, lp2 = rng.normal(size=7), rng.normal(size=5)
    lp2[3] = lp1.max() + 1.0
    np.savez(tmp_path / 'c1.npz', trace=tr1, logp=lp1, names=np.array(names))
    # a chain with its columns in another order is matched by name
    perm = rng.permutation(len(names))
    np.savez(tmp_path / 'c2.npz', trace=tr2[:, perm], logp=lp2, names=np.array(names)[perm])
    s = LA.start_from_chain([str(tmp_path / 'c1.npz'), str(tmp_path / 'c2')], li)
    assert np.array_equal(s, tr2[3])
    assert np.array_equal(LA.start_from_chain(str(tmp_path / 'c1.npz')), tr1[np.argmax(lp1)])
    theta, z = LA.start_point(li, cell_area, s)
    assert np.array_equal(np.r_[theta, z], s)


# ---------------------------------------------------------------- 9. result files
def _parse(path):
    head, vals = {}, []
    for line in open(path).read().splitlines():
        if ' = ' in line:
            n, v = line.split(' = ')
            vals.append((n, float(v)))
        elif line.startswith("Akaike's Information Criterion "):
            head["Akaike's Information Criterion"] = float(line.rsplit(' ', 1)[1])
        elif line.rstrip().endswith(':'):
            head[line.strip()] = None
        elif ': ' in line:
            k, v = line.split(': ', 1)
            head[k] = float(v)
        else:
            head[line.strip()] = None
    return head, vals


def test_result_files_follow_the_reference_lines(site, tmp_path):
    g, li, cell_area = site
    r = LA.find_map(None, li, cell_area, evaluate=_evaluator(g), maxeval=60)
    txt, npz, js = r.save(str(tmp_path / 'map'), {'site': 'test'})
    head, vals = _parse(txt)
    assert list(head) == ['Time elapsed', 'Free stochastic variables', 'Joint log-probability of model',
                          'Max joint log-probability of model', 'Maximum log-likelihood',
                          "Akaike's Information Criterion", '---------------Variable estimates---------------']
    k, lnL = head['Free stochastic variables'], head['Maximum log-likelihood']
    assert k == len(LA.free_names(li)) and head["Akaike's Information Criterion"] == pytest.approx(2 * (k - lnL))
    assert [n for n, _ in vals] == r.names and np.allclose([v for _, v in vals], r.x, rtol=1e-15)
    n = LA.normal_approx(None, li, cell_area, at=r, evaluate=_evaluator(g))
    paths = n.save(str(tmp_path / 'norm'))
    head, vals = _parse(paths[0])
    assert list(head) == ['Time elapsed', 'Free stochastic variables', 'Joint log-probability of model',
                          'Max joint log-probability of model', "Akaike's Information Criterion",
                          '---------------Variable estimates---------------', 'Estimated means:',
                          'Estimated variances:']
    assert [v for _, v in vals[:len(n.names)]] == pytest.approx(list(n.mu), rel=1e-15)
    assert [v for _, v in vals[len(n.names):]] == pytest.approx(list(np.diag(n.C)), rel=1e-15)
    assert head["Akaike's Information Criterion"] == pytest.approx(2 * (n.k - n.lnL))
    with np.load(paths[1]) as f:
        assert np.array_equal(f['C'], n.C) and np.array_equal(f['H'], n.H) and bool(f['pd']) == n.pd
        assert list(f['names']) == n.names and np.array_equal(f['steps'], n.steps)


# ---------------------------------------------------------------- 10. the shared map writer
class _FakeSummary():
    def __init__(self, N=9, days=(0, 2, 3)):
        rng = np.random.default_rng(2)
        self.days = list(days)
        self.thresholds = [1.0, 5.0]
        self.pm = types.SimpleNamespace(days=[10, 11, 12, 13])
        self.total_weight, self.members = 4.0, 3
        self._m = {d: np.where(rng.random((N, N)) < 0.5, 0.0, rng.random((N, N)) * 10) for d in days}

    def mean(self, d):
        return self._m[d]

    def sd(self, d):
        return np.sqrt(self._m[d]) * 0.1

    def exceedance(self, d, k):
        return (self._m[d] >= self.thresholds[k]).astype(float)


def _old_writer(s, outfile):
    """the writer as PredictiveResult.save held it before save_maps was factored out"""
    from scipy import sparse
    out = {}
    labels = []
    for d in s.days:
        label = s.pm.days[d] if d < len(s.pm.days) else d
        labels.append(label)
        maps = [('', s.mean(d)), ('_sd', s.sd(d))]
        maps += [('_pexc%d' % k, s.exceedance(d, k)) for k in range(len(s.thresholds))]
        for suffix, m in maps:
            csr = sparse.csr_matrix(np.where(m >= PP.NEGVAL, m, 0.0))
            out['%s%s_data' % (label, suffix)] = csr.data
            out['%s%s_ind' % (label, suffix)] = csr.indices
            out['%s%s_indptr' % (label, suffix)] = csr.indptr
    out['days'] = np.array(labels)
    np.savez(str(outfile), **out)


def _members(path):
    with zipfile.ZipFile(path) as z:
        return [(i.filename, z.read(i.filename)) for i in z.infolist()]


def test_predictive_files_unchanged_by_the_shared_writer(tmp_path):
    s = _FakeSummary()
    res = PP.PredictiveResult(s, 5, 3, 0, 1.0, [], None, [{'source': None}], s.days)
    npz, js = res.save(str(tmp_path / 'new' / 'pp'), {'site': 'x'})
    _old_writer(s, tmp_path / 'old.npz')
    assert _members(npz) == _members(tmp_path / 'old.npz')      # every member byte for byte, same order
    import json
    meta = json.load(open(js))
    assert meta['site'] == 'x' and meta['predictive']['thresholds'] == [1.0, 5.0]
