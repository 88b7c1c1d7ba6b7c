"""GPU tests of the linearised spread (ps_linspread_*, parasitoids_amd/laplace.py): the centre against
`PopModel.population(d)`, stencil sensitivities, the delta-method variance and exceedances against
numpy / scipy, solver switches, bitwise reproducibility, the MAP + normal approximation end to end on
synthetic observations, and the error paths.  Kalbar wind, R = 128, 6 days unless stated."""
import os
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.abspath(__file__))
DAYS = list(range(6))
# (MODEL_BLOCK name, step) of the stencils tested directly
STENCIL = [('sig_x', 1.0), ('mu_r', 0.05), ('g_aw', 0.05), ('corr_p', 0.01)]


def _wind():
    from parasitoids_amd import ParasitoidModel as PM
    return PM.get_wind_data(os.path.join(ROOT, 'golden', 'data', 'kalbar'), 30, '00:00')


def _pop_model(R=128, ndays=6, **kw):
    from parasitoids_amd.pop_model import PopModel
    wd, days = _wind()
    return PopModel(wd, days[:ndays], domain_info=(10000.0, R), r_number=130000, **kw)


def _theta0():
    from parasitoids_amd import mcmc
    return np.array([m[2] for m in mcmc.MODEL_BLOCK], dtype=np.float64)


def _evaluate(pm, theta, ndays=None):
    from parasitoids_amd import mcmc
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        pm.evaluate(*mcmc.model_args(theta), ndays=ndays, want_stats=False)


def _fields(pm, days=DAYS):
    return np.array([pm.population(d).toarray() for d in days])


def _shift(theta, name, h):
    from parasitoids_amd import mcmc
    t = theta.copy()
    t[[m[0] for m in mcmc.MODEL_BLOCK].index(name)] += h
    return t


def _run_stencil(pm, S, stencil=STENCIL, fields=True):
    """centre at theta0, then +-h on each stencil parameter (param index = position in `stencil`);
    -> (centre fields, {i: (P+, P-)}) read back after every add (or None without `fields`)"""
    t0 = _theta0()
    _evaluate(pm, t0)
    S.set_center()
    P0 = _fields(pm, S.days) if fields else None
    pm_pairs = {}
    for i, (name, h) in enumerate(stencil):
        out = []
        for sign in (1, -1):
            _evaluate(pm, _shift(t0, name, sign * h))
            S.add(i, sign * 0.5 / h)
            if fields:
                out.append(_fields(pm, S.days))
        pm_pairs[i] = tuple(out) if fields else None
    return P0, pm_pairs


def _spd(n, seed=3):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(n, n))
    return A @ A.T + n * np.eye(n)


@pytest.mark.parametrize('prob_model', [False, True])
def test_center_equals_population_bit_for_bit(prob_model):
    from parasitoids_amd.laplace import LinearisedSpread
    pm = _pop_model(prob_model=prob_model)
    with LinearisedSpread(pm, DAYS, 2) as S:
        _evaluate(pm, _theta0())
        S.set_center()
        for d in DAYS:
            assert np.array_equal(S.mean(d), pm.population(d).toarray()), d
        if prob_model:
            assert any(pm.stats[d].delta != 0.0 for d in range(5))
    pm.close()


def test_sensitivities_variance_and_exceedance_against_numpy():
    from scipy.stats import norm
    from parasitoids_amd.laplace import LinearisedSpread
    pm = _pop_model()
    thr = (1.0, 100.0)
    n = len(STENCIL)
    with LinearisedSpread(pm, DAYS, n, thr, names=[s[0] for s in STENCIL]) as S:
        P0, pairs = _run_stencil(pm, S)
        J = []
        for i, (name, h) in enumerate(STENCIL):
            Pp, Pm = pairs[i]
            ref = (Pp - Pm) / (2 * h)
            J.append(ref)
            scale = max(np.abs(Pp).max(), np.abs(Pm).max()) / (2 * h)
            for k, d in enumerate(DAYS):
                got = S.sensitivity(d, name)
                assert np.abs(got - ref[k]).max() <= 1e-14 * scale, (name, d)
            assert np.abs(ref).max() > 0
        assert list(S.info()[2]) == [2] * n
        J = np.array(J)                                  # [param, day, N, N]
        Sig = _spd(n)
        F = np.linalg.cholesky(Sig)
        S.finalize(F)
        Jd = np.array([[S.sensitivity(d, i) for d in DAYS] for i in range(n)])
        var_ref = np.einsum('iduv,ij,jduv->duv', Jd, Sig, Jd)
        for k, d in enumerate(DAYS):
            v = S.variance(d)
            assert np.all(v >= 0)
            assert np.abs(v - var_ref[k]).max() <= 1e-12 * var_ref[k].max(), d
            c = S.mean(d)
            sd = np.sqrt(v)
            for t, th in enumerate(thr):
                with np.errstate(divide='ignore', invalid='ignore'):
                    ref = np.where(sd > 0, norm.sf((th - c) / np.where(sd > 0, sd, 1.0)), (c >= th).astype(float))
                assert np.abs(S.exceedance(d, t) - ref).max() <= 1e-14, (d, th)
            assert np.array_equal(S.sd(d), sd)
        # F = 0: no spread, the exceedance is the indicator of the centre
        S.finalize(np.zeros((n, n)))
        for d in DAYS:
            assert not S.sd(d).any()
            for t, th in enumerate(thr):
                assert np.array_equal(S.exceedance(d, t), (S.mean(d) >= th).astype(float))
    pm.close()


def test_stencil_members_on_different_solvers_in_exact_mode():
    """exact mode keys solvers by kernel extent: large sig_x steps land on other solvers (other streams);
    the handle's events order the adds, and the result equals one built from fields read back later"""
    from parasitoids_amd.laplace import LinearisedSpread
    pm = _pop_model(mode='exact')
    stencil = [('sig_x', 60.0), ('sig_y', 50.0)]
    solvers = set()
    t0 = _theta0()
    with LinearisedSpread(pm, DAYS, 2) as S:
        _evaluate(pm, t0)
        S.set_center()
        solvers.add(id(pm.solver))
        for i, (name, h) in enumerate(stencil):
            for sign in (1, -1):
                _evaluate(pm, _shift(t0, name, sign * h))
                solvers.add(id(pm.solver))
                S.add(i, sign * 0.5 / h)
        assert len(solvers) >= 2
        # the fields only now, every member evaluated again
        for i, (name, h) in enumerate(stencil):
            _evaluate(pm, _shift(t0, name, h))
            Pp = _fields(pm)
            _evaluate(pm, _shift(t0, name, -h))
            Pm = _fields(pm)
            for k, d in enumerate(DAYS):
                ref = (Pp[k] - Pm[k]) / (2 * h)
                scale = max(np.abs(Pp[k]).max(), np.abs(Pm[k]).max()) / (2 * h)
                assert np.abs(S.sensitivity(d, i) - ref).max() <= 1e-14 * scale, (name, d)
        _evaluate(pm, t0)
        assert all(np.array_equal(S.mean(d), pm.population(d).toarray()) for d in DAYS)
    pm.close()


def test_bitwise_reproducible():
    from parasitoids_amd.laplace import LinearisedSpread

    def run():
        pm = _pop_model()
        with LinearisedSpread(pm, [0, 2, 5], len(STENCIL), (1.0,)) as S:
            _run_stencil(pm, S, fields=False)
            S.finalize(np.linalg.cholesky(_spd(len(STENCIL))))
            out = [S.mean(d) for d in S.days] + [S.variance(d) for d in S.days] + [S.exceedance(5, 0)]
            out += [S.sensitivity(2, i) for i in range(len(STENCIL))]
        pm.close()
        return out
    a, b = run(), run()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_map_and_normal_approx_end_to_end(tmp_path):
    from parasitoids_amd import laplace as LA
    from parasitoids_amd import mcmc
    pm = _pop_model(ndays=6, mode='exact')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        li = mcmc.synthetic_locinfo(pm, 128, seed=9)
        cell_area = (10000.0 / 128) ** 2
        start = _theta0()
        start[[m[0] for m in mcmc.MODEL_BLOCK].index('sig_x')] = 200.0
        r = LA.find_map(pm, li, cell_area, start=start, maxeval=25)
        assert r.logp > r.logp_start and r.evaluations <= 25 and r.failed == 0
        days = [0, 3, 5]
        res = LA.normal_approx(pm, li, cell_area, at=r, days=days, thresholds=(1.0, 100.0))
    m = len(LA.FREE_MODEL) - sum(n in res.held for n in LA.FREE_MODEL_NAMES)
    assert res.evaluations == 1 + 2 * m + 2 * m * (m - 1) and res.failed == 0
    assert np.array_equal(res.H, res.H.T) and np.array_equal(res.C, res.C.T)
    S = res.spread
    centered, finalized, adds = S.info()
    assert centered and finalized and list(adds) == [0 if res.steps[i] == 0 else 2 for i in range(len(adds))]
    nm = len(LA.FREE_MODEL)
    # numpy assembly from the stencil fields, each member evaluated again
    post = LA.Posterior(pm, li, cell_area, r.n_periods)
    J = np.zeros((nm, len(days)) + S.mean(0).shape)
    for i in range(nm):
        h = res.steps[i]
        if h == 0:
            continue
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            _evaluate(pm, post.theta(LA.axis_point(res.mu, res.steps, i, 1)[:nm]))
            Pp = _fields(pm, days)
            _evaluate(pm, post.theta(LA.axis_point(res.mu, res.steps, i, -1)[:nm]))
            Pm = _fields(pm, days)
        J[i] = (Pp - Pm) / (2 * h)
        scale = max(np.abs(Pp).max(), np.abs(Pm).max()) / (2 * h)
        for k, d in enumerate(days):
            assert np.abs(S.sensitivity(d, i) - J[i, k]).max() <= 1e-14 * scale, (i, d)
    Jd = np.array([[S.sensitivity(d, i) for d in days] for i in range(nm)])
    U = np.einsum('ik,iduv->kduv', res.F, Jd)
    var = (U ** 2).sum(0)
    Sig = res.C[:nm, :nm]
    var2 = np.einsum('iduv,ij,jduv->duv', Jd, Sig, Jd)
    for k, d in enumerate(days):
        v = S.variance(d)
        assert np.abs(v - var[k]).max() <= 1e-12 * max(var[k].max(), 1e-300), d
        if res.pd:
            assert np.abs(v - var2[k]).max() <= 1e-8 * max(var2[k].max(), 1e-300), d
    _evaluate(pm, r.theta)
    assert all(np.array_equal(S.mean(d), pm.population(d).toarray()) for d in days)
    paths = res.save(str(tmp_path / 'norm'), {'synthetic': True})
    with np.load(paths[2]) as f:
        assert list(f['days']) == [pm.days[d] for d in days]
        assert str(pm.days[3]) + '_sd_data' in f and str(pm.days[5]) + '_pexc1_indptr' in f
    S.close()
    pm.close()


def test_error_paths():
    import ctypes as C
    from parasitoids_amd import _lib as L
    from parasitoids_amd.laplace import LinearisedSpread
    pm = _pop_model()
    with pytest.raises(L.HipError) as e:
        LinearisedSpread(pm, DAYS, 17)
    assert e.value.code == L.PS_ERR_BAD_ARG
    with LinearisedSpread(pm, DAYS, 2, (1.0,)) as S:
        with pytest.raises(L.HipError) as e:          # no centre
            S.mean(0)
        assert e.value.code == L.PS_ERR_STATE
        _evaluate(pm, _theta0())
        S.set_center()
        S.add(0, 1.0)
        with pytest.raises(L.HipError) as e:          # before finalize
            S.variance(1)
        assert e.value.code == L.PS_ERR_STATE
        with pytest.raises(L.HipError) as e:
            S.exceedance(1, 0)
        assert e.value.code == L.PS_ERR_STATE
        S.finalize(np.eye(2))
        S.variance(1)
        S.add(1, -1.0)                                # a later add invalidates the maps
        with pytest.raises(L.HipError) as e:
            S.variance(1)
        assert e.value.code == L.PS_ERR_STATE
        with pytest.raises(L.HipError) as e:
            S.add(2, 1.0)                             # parameter out of range
        assert e.value.code == L.PS_ERR_BAD_ARG
        with pytest.raises(L.HipError) as e:
            S.fetch_slot(6, 0)
        assert e.value.code == L.PS_ERR_BAD_ARG
        _evaluate(pm, _theta0(), ndays=3)             # days 3..5 are not in the last evaluation
        with pytest.raises(ValueError):
            S.set_center()
        with pytest.raises(ValueError):
            S.add(0, 1.0)
    # the memory check: 22 x 2000 slots x 4097^2 cells x 8 B, refused before any allocation
    lib = L.load()
    h = L._VP()
    thr = L.f64([1.0, 2.0, 3.0, 4.0])
    rc = lib.ps_linspread_create(L.default_device(), 4097, 2000, 16, 4, L.p_f64(thr), C.byref(h))
    assert rc == L.PS_ERR_OOM and not h
    assert b'GB' in lib.ps_last_error()
    pm.close()
