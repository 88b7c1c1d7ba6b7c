"""CPU tests of the trace and observation logic of parasitoids_amd/predictive.py: burn / thin and
run-length deduplication, column matching, the observation-rate helper against mcmc.loglik_parts,
reproducible predictive draws.  No device: expected observations come from `evaluate=`."""
import types

import numpy as np
import pytest

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


def _names(li):
    return ([m[0] for m in mcmc.MODEL_BLOCK] + [m[0] for m in mcmc.NUISANCE] + ['A_collected']
            + ['sent_obs_probs_%s' % k for k in li.sent_ids])


def _trace(li, cell_area, lengths, seed=3):
    """rows in runs of identical model parameters with the given lengths; nuisance columns differ
    on every row"""
    rng = np.random.default_rng(seed)
    t0 = np.array([m[2] for m in mcmc.MODEL_BLOCK])
    sp = mcmc.initial_sent_obs_probs(li, cell_area)
    rows = []
    for r, n in enumerate(lengths):
        theta = t0 * (1.0 + 0.01 * r)
        for _ in range(n):
            nu = np.array([m[2] for m in mcmc.NUISANCE]) * (1 + 0.05 * rng.random(3))
            rows.append(np.concatenate([theta, nu, [2000.0], sp * (1 + 0.05 * rng.random(len(sp)))]))
    return np.array(rows)


def _evaluator(g, calls=None, reject=None):
    base = ([g['rel0'], g['rel1']], [g['sen0'], g['sen1']], g['grid'])
    t0 = np.array([m[2] for m in mcmc.MODEL_BLOCK])

    def evaluate(theta):
        if calls is not None:
            calls.append(np.array(theta))
        f = float(np.exp(-((theta / t0 - 1.0) ** 2).sum()))
        if reject is not None and reject(theta):
            return None
        return ([f * r for r in base[0]], [f * s for s in base[1]], f * base[2])
    return evaluate


def test_runs_of_identical_parameters_are_one_weighted_evaluation(golden):
    g = golden('g9_bayes_funcs')
    li, cell_area = _locinfo(g)
    lengths = [3, 1, 4, 2, 6, 1]
    tr = _trace(li, cell_area, lengths)
    names = _names(li)
    calls = []
    res = PP.posterior_predictive(None, (tr, names), evaluate=_evaluator(g, calls))
    assert res.rows == sum(lengths) and res.evaluations == len(lengths) == len(calls)
    assert [w for _c, _f, w in res.runs] == lengths and res.failed == 0
    assert res.summary is None
    # burn 2, thin 2 over rows 0..16: kept rows 2, 4, ..., 16 -> runs of the thinned chain
    res = PP.posterior_predictive(None, [(tr, names)], burn=2, thin=2, evaluate=_evaluator(g))
    rows = tr[2::2]
    _, want = PP.runs(tr, list(range(15)), 2, 2)
    assert res.rows == len(rows) == 8
    assert [(f, w) for _c, f, w in res.runs] == want
    assert sum(w for _f, w in want) == len(rows)
    for f, w in want:
        assert all(np.array_equal(rows[f + i, :15], rows[f, :15]) for i in range(w))
        assert f + w == len(rows) or not np.array_equal(rows[f + w, :15], rows[f, :15])
    # two chains: runs never cross a chain boundary, each chain keeps its own burn / thin
    res = PP.posterior_predictive(None, [(tr, names), (tr[::-1], names)], burn=1, evaluate=_evaluator(g))
    assert res.rows == 2 * (len(tr) - 1) and sorted({c for c, _f, _w in res.runs}) == [0, 1]
    # a rejected evaluation is skipped and counted
    bad = np.array([m[2] for m in mcmc.MODEL_BLOCK]) * 1.02
    res = PP.posterior_predictive(None, (tr, names), locinfo=li,
                                  evaluate=_evaluator(g, reject=lambda t: np.array_equal(t, bad)))
    assert res.failed == 1 and res.evaluations == len(lengths)
    assert [w for _c, _f, w in res.runs] == [3, 1, 2, 6, 1]
    assert res.observations['grid']['q50'].shape == li.grid_obs.ravel().shape


def test_wrong_column_names_raise(golden, tmp_path):
    g = golden('g9_bayes_funcs')
    li, cell_area = _locinfo(g)
    tr = _trace(li, cell_area, [2, 2])
    names = _names(li)
    wrong = list(names)
    wrong[names.index('sig_x')] = 'sigma_x'
    with pytest.raises(ValueError, match='different model'):
        PP.posterior_predictive(None, (tr, wrong), evaluate=_evaluator(g))
    np.savez(tmp_path / 'c.npz', trace=tr, names=np.array(wrong))
    with pytest.raises(ValueError, match='different model'):
        PP.posterior_predictive(None, str(tmp_path / 'c.npz'), evaluate=_evaluator(g))
    # the observation predictive needs the site's sentinel columns too
    nosent = [n if not n.startswith('sent_obs_probs_C') else 'other' for n in names]
    with pytest.raises(ValueError, match='different model'):
        PP.posterior_predictive(None, (tr, nosent), locinfo=li, evaluate=_evaluator(g))
    # columns are matched by name, not position
    perm = np.random.default_rng(0).permutation(len(names))
    a = PP.posterior_predictive(None, (tr, names), locinfo=li, evaluate=_evaluator(g), seed=5)
    b = PP.posterior_predictive(None, (tr[:, perm], [names[i] for i in perm]), locinfo=li,
                                evaluate=_evaluator(g), seed=5)
    assert a.runs == b.runs
    for grp in ('release', 'sentinel', 'grid'):
        assert np.array_equal(a.observations[grp]['q95'], b.observations[grp]['q95'])


def test_rate_helper_reproduces_loglik_parts(golden):
    g = golden('g9_bayes_funcs')
    li, cell_area = _locinfo(g)
    c = mcmc.observation_cache(li)
    expected = ([g['rel0'] * 1.3, g['rel1'] * 0.7], [g['sen0'], g['sen1'] * 1.1], g['grid'] * 0.9)
    nuis = (0.6, 0.07, 0.004)
    sp = mcmc.initial_sent_obs_probs(li, cell_area) * np.array([1.0, 1.2, 0.8])
    rel, sen, grid = PP.observation_rates(expected, li, nuis, sp)
    parts = mcmc.loglik_parts(expected, li, nuis, sp)
    mine = (sum(mcmc.poisson_loglik(c['rel'][i], r, c['rel_lg'][i]) for i, r in enumerate(rel)),
            sum(mcmc.poisson_loglik(c['sen'][i], s, c['sen_lg'][i]) for i, s in enumerate(sen)),
            mcmc.poisson_loglik(c['grid'], grid, c['grid_lg']))
    assert np.all(np.isfinite(parts))
    assert mine == parts


def test_predictive_quantiles_are_reproducible(golden, tmp_path):
    g = golden('g9_bayes_funcs')
    li, cell_area = _locinfo(g)
    tr = _trace(li, cell_area, [5, 3, 7, 2])
    names = _names(li)
    np.savez(tmp_path / 'chain.npz', trace=tr, names=np.array(names))
    kw = dict(locinfo=li, cell_area=cell_area, evaluate=_evaluator(g))
    a = PP.posterior_predictive(None, str(tmp_path / 'chain.npz'), seed=7, **kw)
    b = PP.posterior_predictive(None, (tr, names), seed=7, **kw)
    d = PP.posterior_predictive(None, (tr, names), seed=8, **kw)
    differs = False
    for grp in ('release', 'sentinel', 'grid'):
        A, B = a.observations[grp], b.observations[grp]
        for key in ('mean_rate', 'q05', 'q50', 'q95'):
            assert np.array_equal(A[key], B[key]), (grp, key)
        assert A['p_total'] == B['p_total'] and 0.0 <= A['p_total'] <= 1.0
        assert np.all(A['q05'] <= A['q50']) and np.all(A['q50'] <= A['q95'])
        differs = differs or not np.array_equal(A['q95'], d.observations[grp]['q95'])
    assert differs
    # the mean rate is the row average of the rate helper's output
    rows = []
    ev = _evaluator(g)
    for r in tr:
        rows.append(PP._flat([PP.observation_rates(ev(r[:15]), li, r[15:18], r[19:])[2]]))
    assert np.allclose(a.observations['grid']['mean_rate'], np.mean(rows, 0), rtol=1e-14, atol=0)
