"""CPU tests of the reweighting for new observations (predictive.ReweightedSummary and its host helpers): the numpy
reference loop (reweight_ref) against the plain two-pass definitions with normalised weights, the probe
log-likelihoods against scipy, the run formula, the weight diagnostics on hand-made weights, and every refusal
that needs no device."""
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import reweight_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = [1, 3, 1, 2, 1, 4]
THR = [0.5, 4.0]
LAMS = {'flat': [0.0] * 6,
        'swing': [0.0, -1.5, 2.25, 2.25, -800.0, 1.0],
        'late': [-math.inf, 0.5, -0.25, 3.0, 1.0, -2.0],
        'huge': [-700.0, 650.0, 649.0, -300.0, 651.5, 650.5]}


def _fields(seed, shape=(3, 9, 9)):
    rng = np.random.default_rng(seed)
    out = []
    for _ in WEIGHTS:
        f = 10.0 ** rng.uniform(-2, 2, size=shape)
        f[rng.random(shape) < 0.6] = 0.0
        out.append(f)
    return out


def _close(got, want, scale):
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15 * scale)


def test_the_loop_matches_the_two_pass_definitions():
    fields = _fields(5)
    names = list(LAMS)
    st = RR.new_state(fields[0].shape, THR, len(names))
    for m, (f, w) in enumerate(zip(fields, WEIGHTS)):
        RR.add(st, f, [LAMS[n][m] for n in names], w)
    for sc, n in zip(st, names):
        mu, var, exc = RR.two_pass(fields, WEIGHTS, LAMS[n], THR)
        scale = np.abs(mu).max()
        _close(RR.mean(sc), mu, scale)
        _close(RR.variance(sc), var, scale ** 2)
        for k in range(len(THR)):
            _close(RR.exceedance(sc, k), exc[k], 1.0)
        assert sc['ref'] == max(LAMS[n]) and 0 < sc['W'] <= sum(WEIGHTS)
        lw = np.log(np.sum(np.asarray(WEIGHTS) * np.exp(np.asarray(LAMS[n]) - max(LAMS[n])))) + max(LAMS[n])
        assert abs(RR.log_total_weight(sc) - lw) <= 1e-12 * abs(lw)
    assert [sc['skipped'] for sc in st] == [0, 1, 1, 1] and [sc['members'] for sc in st] == [6, 5, 5, 5]
    # the flat scenario is the plain weighted Welford: integer W
    assert st[0]['W'] == sum(WEIGHTS) and st[0]['ref'] == 0.0


def test_the_reference_merge_matches_one_pass():
    fields = _fields(6)
    names = list(LAMS)
    one = RR.new_state(fields[0].shape, THR, len(names))
    a = RR.new_state(fields[0].shape, THR, len(names))
    b = RR.new_state(fields[0].shape, THR, len(names))
    for m, (f, w) in enumerate(zip(fields, WEIGHTS)):
        lam = [LAMS[n][m] for n in names]
        RR.add(one, f, lam, w)
        RR.add(a if m < 3 else b, f, lam, w)
    RR.merge(a, b)
    for sa, so, n in zip(a, one, names):
        scale = np.abs(so['mean']).max()
        _close(RR.mean(sa), RR.mean(so), scale)
        _close(RR.variance(sa), RR.variance(so), scale ** 2)
        for k in range(len(THR)):
            _close(RR.exceedance(sa, k), RR.exceedance(so, k), 1.0)
        assert sa['ref'] == so['ref']
        if n != 'huge':     # there the second half starts 950 below the first's reference: a member, not a skip
            assert (sa['members'], sa['skipped']) == (so['members'], so['skipped'])
    empty = RR.new_state(fields[0].shape, THR, len(names))
    RR.merge(empty, b)
    for se, sb in zip(empty, b):
        assert np.array_equal(se['mean'], sb['mean']) and np.array_equal(se['q'], sb['q']) and se['W'] == sb['W']


def test_probe_loglik_against_scipy():
    from scipy.stats import poisson
    from parasitoids_amd.predictive import probe_loglik, probes_loglik, check_probes
    for n, mu in ((0, 0.3), (3, 2.5), (14, 9.1), (1, 1e-3), (50, 61.0), (3, 130.0), (0, 45.0)):
        for rate in (1.0, 0.5, 1e-3):
            got = probe_loglik('count', rate, mu / rate, n)
            want = poisson.logpmf(n, rate * (mu / rate))
            assert abs(got - want) <= 1e-13 * abs(want), (n, mu, rate)
            assert got == RR.probe_loglik('count', rate, mu / rate, n)
    # log1p(-exp(-mu)) itself is good to 1e-13 only from mu = 0.01 up: below, 1 - exp(-mu) has lost too many digits
    for mu in (0.01, 0.1, 0.5, 0.69, 0.7, 1.0, 3.0, 10.0, 40.0, 800.0):
        got = probe_loglik('found', 0.5, mu / 0.5)
        assert got == RR.probe_loglik('found', 0.5, mu / 0.5)
        want = np.log1p(-np.exp(-(0.5 * (mu / 0.5))))
        assert abs(got - want) <= 1e-13 * abs(want), mu
        assert probe_loglik('none', 0.5, mu / 0.5) == -(0.5 * (mu / 0.5))
    # mu = 0: a cell the member holds nothing in
    assert probe_loglik('count', 2.0, 0.0, 0) == 0.0 == poisson.logpmf(0, 0.0)
    assert probe_loglik('count', 2.0, 0.0, 3) == -math.inf == poisson.logpmf(3, 0.0)
    assert probe_loglik('none', 2.0, 0.0) == 0.0
    with np.errstate(divide='ignore'):
        assert probe_loglik('found', 2.0, 0.0) == -math.inf == np.log1p(-np.exp(-0.0))
    with pytest.raises(ValueError):
        probe_loglik('seen', 1.0, 1.0)
    # a scenario's log-weight: the sum in list order
    given = [(0, 0, 1, 'count', 1e-3, 3), (3000, 0, 2, 'found', 0.5), (0, -2000, 4, 'none', 0.25)]
    probes = check_probes(given, 10000.0, 64, 6)
    vals = [2100.0, 0.7, 3.0]
    want = ((0.0 + probe_loglik('count', 1e-3, 2100.0, 3)) + probe_loglik('found', 0.5, 0.7)) + probe_loglik('none', 0.25, 3.0)
    assert probes_loglik(probes, vals) == want == RR.probes_loglik(given, vals)
    assert probes_loglik(probes, [2100.0, 0.0, 3.0]) == -math.inf
    assert [(p['row'], p['col']) for p in probes] == [(64, 64), (64, 64 + 19), (64 + 13, 64)]


def test_the_run_formula():
    from parasitoids_amd.predictive import run_log_weight
    for v in (0.0, -3.7, 812.25, -1e4):
        for n in (1, 2, 7):
            assert run_log_weight([v] * n) == v == RR.run_log_weight([v] * n)
    assert run_log_weight([-math.inf] * 3) == -math.inf
    assert run_log_weight([-math.inf]) == -math.inf
    got = run_log_weight([0.0, -math.inf, math.log(3.0)])
    assert abs(got - math.log(4.0 / 3.0)) < 1e-15
    assert abs(run_log_weight([-1000.0, -1001.0]) - (-1000.0 + math.log((1 + math.exp(-1.0)) / 2))) < 1e-12


def test_diagnostics_on_hand_made_weights():
    from parasitoids_amd.predictive import reweight_diagnostics
    d = reweight_diagnostics(np.log([1.0, 1.0, 1.0, 1.0]) + 123.0)
    assert d['rows'] == 4 and d['skipped_rows'] == 0 and d['ess'] == 4.0 and d['max_share'] == 0.25
    assert abs(d['log_mean_weight'] - 123.0) < 1e-13
    d = reweight_diagnostics([math.log(3.0), 0.0, -math.inf, -5000.0])
    assert d['rows'] == 4 and d['skipped_rows'] == 2
    assert abs(d['ess'] - 16.0 / 10.0) < 1e-14 and abs(d['max_share'] - 0.75) < 1e-15
    assert abs(d['log_mean_weight'] - math.log(1.0)) < 1e-15
    assert d == RR.diagnostics([math.log(3.0), 0.0, -math.inf, -5000.0])
    d = reweight_diagnostics([0.0] + [-math.inf] * 9)
    assert d['ess'] == 1.0 and d['max_share'] == 1.0 and d['skipped_rows'] == 9
    d = reweight_diagnostics([-math.inf] * 3)
    assert d['ess'] == 0.0 and d['skipped_rows'] == 3 and d['log_mean_weight'] == -math.inf


def test_the_scale_bookkeeping_keeps_every_weight_below_the_run_length():
    """the r / omega rules of the class, replayed by the reference on the same log-weights"""
    for name, lams in LAMS.items():
        ref = -math.inf
        for lam, w in zip(lams, WEIGHTS):
            r, om, new = RR.scale(ref, lam, w)
            assert 0.0 <= r <= 1.0 and 0.0 <= om <= w
            if om > 0.0:
                ref = new
        assert ref == max(lams)


BAD_PROBES = [
    ('not a list', 5),
    ('empty', []),
    ('too short', [(0, 0, 1, 'none')]),
    ('too long', [(0, 0, 1, 'count', 1.0, 3, 4)]),
    ('kind', [(0, 0, 1, 'seen', 1.0)]),
    ('text position', [('a', 0, 1, 'none', 1.0)]),
    ('infinite position', [(math.inf, 0, 1, 'none', 1.0)]),
    ('fractional day', [(0, 0, 1.5, 'none', 1.0)]),
    ('negative day', [(0, 0, -1, 'none', 1.0)]),
    ('day past the model', [(0, 0, 6, 'none', 1.0)]),
    ('zero rate', [(0, 0, 1, 'none', 0.0)]),
    ('negative rate', [(0, 0, 1, 'found', -1.0)]),
    ('nan rate', [(0, 0, 1, 'found', math.nan)]),
    ('count without n', [(0, 0, 1, 'count', 1.0)]),
    ('negative n', [(0, 0, 1, 'count', 1.0, -1)]),
    ('fractional n', [(0, 0, 1, 'count', 1.0, 2.5)]),
    ('n with none', [(0, 0, 1, 'none', 1.0, 2)]),
    ('outside east', [(10100, 0, 1, 'none', 1.0)]),
    ('outside south', [(0, -10100, 1, 'none', 1.0)]),
]


@pytest.mark.parametrize('why,probes', BAD_PROBES, ids=[b[0] for b in BAD_PROBES])
def test_check_probes_refuses(why, probes):
    from parasitoids_amd.predictive import check_probes
    with pytest.raises(ValueError):
        check_probes(probes, 10000.0, 64, 6)


def test_check_probes_accepts_the_edge_of_the_domain():
    from parasitoids_amd.predictive import check_probes
    got = check_probes([(10000, -10000, 5, 'count', 2, 0), (-10000, 10000, 0, 'found', 0.1)], 10000.0, 64, 6)
    assert [(p['row'], p['col'], p['day'], p['n']) for p in got] == [(128, 128, 5, 0), (0, 0, 0, None)]
    assert 'row' not in check_probes([(1e9, 0, 50, 'none', 1.0)], None, None)[0]


class _Model(types.SimpleNamespace):
    """what the checks read of a PopModel; an evaluation is a failure of the test"""

    def evaluate(self, *a, **k):
        self.calls.append(a)
        raise RuntimeError('the model was evaluated')


def _model(ndays=6, R=64):
    return _Model(rad_dist=10000.0, rad_res=R, days=list(range(100, 100 + ndays)), r_number=130000,
                  prob_model=False, device=None, solver=None, calls=[])


def test_posterior_predictive_refuses_a_bad_reweight_before_evaluating():
    from parasitoids_amd.predictive import posterior_predictive, model_names
    names = model_names()
    trace = np.zeros((12, len(names)))
    chain = (trace, names)
    pm = _model()
    good = dict(probes=[(0, 0, 1, 'none', 1.0)])
    z = np.zeros(12)
    bad = [5, {}, {'a': 5}, {'a': {}}, {'a': dict(probes=[(0, 0, 1, 'none', 1.0)], log_weights=[z])},
           {'a': dict(probes=[(0, 0, 1, 'none', 1.0)], extra=1)},
           {'a': good, 'b': good, 'c': good, 'd': good, 'e': good},
           {'a': good, 'options': dict(min_ess=-1)}, {'a': good, 'options': dict(ess=5)},
           {'a': dict(log_weights=[np.zeros(11)])}, {'a': dict(log_weights=[np.zeros(13)])},
           {'a': dict(log_weights=[z, z])}, {'a': dict(log_weights=[np.zeros((12, 1))])},
           {'a': dict(log_weights=[np.full(12, np.nan)])}, {'a': dict(log_weights=[np.full(12, np.inf)])},
           {'a': dict(log_weights=5)}]
    bad += [{'a': dict(probes=p)} for _why, p in BAD_PROBES]
    for rw in bad:
        with pytest.raises(ValueError):
            posterior_predictive(pm, chain, reweight=rw)
    # burn and thin count: 12 rows, burn 2, thin 2 leaves 5
    with pytest.raises(ValueError, match='5 rows after burn and thin'):
        posterior_predictive(pm, chain, burn=2, thin=2, reweight={'a': dict(log_weights=[z])})
    with pytest.raises(ValueError, match='not with evaluate='):
        posterior_predictive(pm, chain, evaluate=lambda theta: None, reweight={'a': good})
    for thr in ((0.0,), (10.0, 1.0)):
        with pytest.raises(ValueError, match='finite and > 0|strictly increasing'):
            posterior_predictive(pm, chain, thresholds=thr, reweight={'a': good})
    with pytest.raises(ValueError, match='1..32 days'):
        posterior_predictive(_model(ndays=40), chain, reweight={'a': good})
    assert not pm.calls


def test_check_reweight_keeps_what_was_given():
    from parasitoids_amd.predictive import check_reweight, check_reweight_rows, DEFAULT_MIN_ESS
    z = np.zeros(4)
    plan = check_reweight({'trap': dict(probes=[(0, 0, 1, 'count', 1e-3, 3)]), 'flat': dict(log_weights=[z, z]),
                           'options': dict(min_ess=7)}, 10000.0, 64, 6)
    assert plan['names'] == ['trap', 'flat'] and plan['kinds'] == ['probes', 'log_weights'] and plan['min_ess'] == 7.0
    assert plan['given'] == [[[0, 0, 1, 'count', 1e-3, 3]], None] and plan['probes'][0][0]['row'] == 64
    check_reweight_rows(plan, [4, 4])
    with pytest.raises(ValueError, match='2 chains'):
        check_reweight_rows(plan, [4])
    assert check_reweight({'a': dict(log_weights=[z])})['min_ess'] == DEFAULT_MIN_ESS == 50.0


def test_the_script_refuses_a_bad_reweight_flag():
    """refused by the argument parser, before the package is imported"""
    script = os.path.join(ROOT, 'scripts', 'run_predictive.py')
    for flag in (['--reweight', 'trap'], ['--reweight', 'trap:0,0,1,seen,1'], ['--reweight', 'trap:0,0,1,count,1'],
                 ['--reweight-file', 'weights.npy'],
                 ['--reweight', 'a:0,0,1,none,1', '--reweight', 'a:0,0,1,none,1']):
        r = subprocess.run([sys.executable, script, '--synthetic'] + flag, capture_output=True, text=True)
        assert r.returncode == 2 and 'reweight' in r.stderr, (flag, r.stderr[-300:])


def test_the_reweight_entry_points_are_declared_and_bound():
    from parasitoids_amd import _lib
    names = {'ps_wsum_' + n for n in ('create', 'add', 'add_project', 'add_sites', 'add_peak', 'merge', 'info', 'fetch',
                                      'reset', 'prof', 'destroy')}
    assert names <= set(_lib.SIGNATURES)
    header = open(os.path.join(ROOT, 'include', 'parasitoid_hip.h')).read()
    lib = _lib.load()
    for n in names:
        assert n + '(' in header and hasattr(lib, n), n
