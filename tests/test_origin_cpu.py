"""CPU tests of the origin maps: check_origin's acceptances and every refusal, the host functions of
predictive.OriginMaps on hand-made planes (normalisation, region ties, hypothesis marginals, Bayes factor, a prior
with -inf cells), the float64 restatement (origin_ref) against its 40-digit version within the bounds of DESIGN 7y,
merge against a single pass, log_weights against check_reweight, the twin experiment, the driver's wiring and the
command line, and the host emulation of the device logic (tests/host/origin_emul.cpp over csrc/ps_origin_core.h)
under the sanitizers."""
import math
import os
import subprocess
import types
import warnings

import numpy as np
import pytest

import origin_ref as OR
from parasitoids_amd import predictive as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 10000.0 / 32
F1 = [(2 * RES, 3 * RES, 3, 'count', 0.02, 2), (-4 * RES, RES, 4, 'found', 0.05), (0.0, 0.0, 1, 'none', 0.01)]


def test_check_origin_accepts():
    plan = PR.check_origin(F1, 10000.0, 32, 6)
    assert plan['hypotheses'] == [(1.0, 0)] and plan['lags'] == [0] and plan['groups'] == [0]
    assert plan['days'] == [1, 3, 4] and plan['slots'] == [1, 2, 0] and plan['levels'] == [0.5, 0.95]
    assert plan['prior'] is None and plan['given'] == [list(f) for f in F1]
    assert [(f['row'], f['col']) for f in plan['findings']] == [(29, 34), (31, 28), (32, 32)]
    plan = PR.check_origin(dict(findings=F1, amounts=[0.1, 1, 10], lags=[0, 2]), 10000.0, 32, 6)
    assert plan['hypotheses'] == [(0.1, 0), (0.1, 2), (1.0, 0), (1.0, 2), (10.0, 0), (10.0, 2)]
    assert plan['lags'] == [0, 2] and plan['groups'] == [0, 1, 0, 1, 0, 1]
    plan = PR.check_origin(dict(findings=F1, hypotheses=[(2.0, 3), (0.5, 1)], levels=[0.9]), 10000.0, 32, 6)
    assert plan['hypotheses'] == [(2.0, 3), (0.5, 1)] and plan['lags'] == [1, 3] and plan['groups'] == [1, 0]
    prior = np.zeros((65, 65))
    prior[:, :10] = -np.inf
    plan = PR.check_origin(dict(findings=F1, prior=prior), 10000.0, 32, 6)
    assert np.array_equal(plan['prior'], prior)
    assert PR.check_origin(F1, None, None)['findings'][0].get('row') is None       # no model at hand
    assert PR.parse_origin('625,937.5,3,count,0.02,2; -1250,312.5,4,found,0.05') == \
        [(625.0, 937.5, 3, 'count', 0.02, 2), (-1250.0, 312.5, 4, 'found', 0.05)]
    req = PR.origin_request('0,0,1,none,0.5', '0.1,1', '0,1', '0.8', '', 10000.0, 32)
    assert req == dict(findings=[(0.0, 0.0, 1, 'none', 0.5)], amounts=[0.1, 1.0], lags=[0, 1], levels=[0.8])


@pytest.mark.parametrize('arg, word', [
    ([], 'at least one'),
    ([(0, 0, 1, 'seen', 1.0)], "finding 0: kind 'seen'"),
    ([(0, 0, 1, 'count', 1.0)], 'finding 0'),
    ([(0, 0, 9, 'none', 1.0)], 'day 9'),
    ([(1e6, 0, 1, 'none', 1.0)], 'outside'),
    ([(0, 0, 1, 'none', 0.0)], 'rate'),
    ([(0, 0, 1, 'none', 1.0)] * 65, '65 findings'),
    (dict(findings=F1, sites=[]), 'keys'),
    (dict(amounts=[1]), 'keys'),
    (dict(findings=F1, amounts=[1], hypotheses=[(1, 0)]), 'not both'),
    (dict(findings=F1, hypotheses=[]), '0 hypotheses'),
    (dict(findings=F1, amounts=list(range(1, 10))), '9 hypotheses'),
    (dict(findings=F1, hypotheses=[(1.0,)]), 'hypothesis 0'),
    (dict(findings=F1, hypotheses=[(1.0, 0.5)]), 'hypothesis 0'),
    (dict(findings=F1, amounts=[0.0]), 'amount 0.0'),
    (dict(findings=F1, amounts=[float('nan')]), 'amount'),
    (dict(findings=F1, lags=[-1]), 'negative'),
    (dict(findings=F1, lags=[6]), 'beyond'),
    (dict(findings=F1, lags=[5]), 'after the last finding'),
    (dict(findings=F1, hypotheses=[(1.0, 0), (1, 0)]), 'repeats'),
    (dict(findings=F1, lags=[0, 1, 2, 3, 4]), '5 different lags'),
    (dict(findings=F1, prior=np.zeros((64, 65))), 'shape'),
    (dict(findings=F1, prior=np.full((65, 65), np.nan)), 'NaN'),
    (dict(findings=F1, prior=np.full((65, 65), -np.inf)), 'excludes every cell'),
    (dict(findings=F1, levels=[0.0]), '(0, 1]'),
    (dict(findings=F1, levels=[]), 'at least one level'),
])
def test_check_origin_refuses(arg, word):
    with pytest.raises(ValueError, match='origin') as e:
        PR.check_origin(arg, 10000.0, 32, 6)
    assert word in str(e.value), str(e.value)


def test_check_origin_refuses_too_many_days():
    many = [(0, 0, d, 'none', 1.0) for d in range(33)]
    with pytest.raises(ValueError, match='33 different days'):
        PR.check_origin(many, 10000.0, 32, 40)
    for bad in ('1,2,3', '1,2,x,none,1', ''):
        with pytest.raises(ValueError):
            PR.parse_origin(bad)
    with pytest.raises(ValueError, match='amounts'):
        PR.origin_request('0,0,1,none,0.5', 'a,b')


# ---------------------------------------------------------------- the host functions on hand-made planes
def test_evidence_posterior_and_region_on_hand_made_planes():
    A = np.array([[0.0, -1.0], [-np.inf, math.log(2.0)]])
    S = np.array([[4.0, 2.0], [0.0, 1.0]])
    E = PR.origin_log_evidence(A, S, 4)
    assert E[0, 0] == 0.0 and E[1, 0] == -np.inf and abs(E[0, 1] - (-1.0 + math.log(0.5))) < 1e-15
    assert abs(E[1, 1] - math.log(0.5)) < 1e-15
    with np.errstate(divide='ignore'):
        E2 = np.stack([np.log(np.array([[1.0, 2.0], [0.0, 1.0]])), np.log(np.array([[2.0, 2.0], [0.0, 0.0]]))])
        lp, lq = np.log(np.array([[1.0, 0.5], [1.0, 0.0]])), np.log(np.array([[1.0, 1.0], [0.0, 1.0]]))
    P = PR.origin_posterior(E2)
    assert np.allclose(P, np.array([[[1, 2], [0, 1]], [[2, 2], [0, 0]]]) / 8.0, atol=1e-16) and abs(P.sum() - 1) < 1e-15
    assert np.array_equal(P, OR.posterior(E2))
    Pp = PR.origin_posterior(E2, lp)                              # a -inf cell of the prior, also where E is -inf
    assert np.allclose(Pp, np.array([[[1, 1], [0, 0]], [[2, 1], [0, 0]]]) / 5.0, atol=1e-16)
    assert not np.isnan(PR.origin_posterior(E2, lq)).any()                  # -inf + -inf
    with pytest.raises(ValueError, match='no candidate cell'):
        PR.origin_posterior(np.full((1, 2, 2), -np.inf))
    m = PR.origin_hypothesis_masses(P, [(0.5, 0), (0.5, 2)])
    assert [h['mass'] for h in m['hypotheses']] == [0.5, 0.5] and m['amounts'] == [{'amount': 0.5, 'mass': 1.0}]
    assert m['lags'] == [{'lag': 0, 'mass': 0.5}, {'lag': 2, 'mass': 0.5}]
    # the region: descending mass, ties by the smaller linear index, the smallest set that reaches the level
    mass = np.array([[0.1, 0.3, 0.1], [0.3, 0.1, 0.1]])
    assert PR.origin_region(mass, 0.3).tolist() == [[0, 1, 0], [0, 0, 0]]
    assert PR.origin_region(mass, 0.31).tolist() == [[0, 1, 0], [1, 0, 0]]
    assert PR.origin_region(mass, 0.65).tolist() == [[1, 1, 0], [1, 0, 0]]
    assert PR.origin_region(mass, 1.0).sum() == 6 and PR.origin_region(mass, 0.5).dtype == np.int8
    for level in (0.3, 0.31, 0.65, 0.8, 1.0):
        assert np.array_equal(PR.origin_region(mass, level), OR.region(mass, level))
    with pytest.raises(ValueError):
        PR.origin_region(mass, 0.0)


class _Stub(PR.OriginMaps):
    """the host side of OriginMaps over planes given by hand: no device, no library"""

    def __init__(self, A, S, W, hypotheses, rows=None, weights=None, prior=None):
        self._A, self._S, self._W = np.asarray(A, dtype=np.float64), np.asarray(S, dtype=np.float64), W
        self.pairs, self.log_prior, self.levels = hypotheses, prior, [0.5, 0.95]
        self.N = self._A.shape[-1]
        self.pm = types.SimpleNamespace(rad_dist=1000.0, rad_res=self.N // 2)
        self.cell_area = (1000.0 / (self.N // 2)) ** 2
        self._rows, self._weights = rows, weights

    total_weight = property(lambda self: float(self._W))
    members = property(lambda self: len(self._weights))

    def plane(self, what, h):
        return {'A': self._A, 'S': self._S}[what][h]

    def member_rows(self):
        return np.asarray(self._rows, dtype=np.float64), np.asarray(self._weights, dtype=np.int64)

    def close(self):
        pass


def test_mode_at_bayes_factor_and_warnings_through_the_class():
    N = 5
    A = np.full((3, N, N), -np.inf)
    S = np.zeros((3, N, N))
    A[0, 1, 1], S[0, 1, 1] = math.log(1.0), 2.0
    A[1, 1, 1], S[1, 1, 1] = math.log(3.0), 2.0
    A[1, 3, 2], S[1, 3, 2] = math.log(4.0), 1.0
    A[2, 3, 2], S[2, 3, 2] = math.log(8.0), 2.0
    rows = [[[0.0, 1.0]] * 3] * 60
    om = _Stub(A, S, 2, [(0.1, 0), (1.0, 0), (10.0, 0)], rows, [1] * 60)
    P = om.posterior()
    assert np.allclose(P[1, 1], 4.0 / 14.0) and np.allclose(P[3, 2], 10.0 / 14.0) and abs(P.sum() - 1) < 1e-15
    assert np.allclose(om.posterior(2)[3, 2], 8.0 / 14.0)
    with pytest.warns(UserWarning, match='outermost amount 10'):
        mode = om.mode()
    assert (mode['row'], mode['col'], mode['hypothesis'], mode['amount'], mode['lag']) == (3, 2, 2, 10.0, 0)
    assert (mode['east'], mode['north']) == (0.0, -500.0) and np.allclose(mode['mass'], 8.0 / 14.0)
    assert np.allclose(om.at(0.0, -500.0), 10.0 / 14.0) and om.at(500.0, 500.0) == 0.0
    assert om.region(0.5).sum() == 1 and om.region(0.95).sum() == 2 and om.area(0.95) == 2 * 500.0 ** 2
    # our site (-500, 500) -> cell (1, 1) or theirs (0, -500) -> cell (3, 2): the hypotheses averaged
    bf = om.log_bayes_factor((-500.0, 500.0), (0.0, -500.0))
    assert abs(bf - math.log(4.0 / 10.0)) < 1e-15
    assert om.log_bayes_factor((-500.0, 500.0), (500.0, 500.0)) == np.inf
    assert math.isnan(om.log_bayes_factor((500.0, 500.0), (1000.0, 1000.0)))
    masses = om.hypotheses()
    assert np.allclose([h['mass'] for h in masses['hypotheses']], [1 / 14.0, 5 / 14.0, 8 / 14.0])
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        d = om.diagnostics()                             # 60 equal rows: no warning
    assert d['rows'] == 60 and abs(d['ess'] - 60.0) < 1e-9
    # an inversion that hangs on two members of the chain needs saying
    few = _Stub(A, S, 2, [(1.0, 0)] * 3, [[[0.0, 1.0]] * 3] * 2 + [[[-50.0, 1.0]] * 3] * 58, [1] * 60)
    with pytest.warns(UserWarning, match='effective sample'):
        d = few.diagnostics()
    assert d['ess'] < 2.01 and d['ess'] < PR.DEFAULT_MIN_ESS
    # a prior with -inf cells takes their mass away
    prior = np.zeros((N, N))
    prior[3, 2] = -np.inf
    masked = _Stub(A, S, 2, [(0.1, 0), (1.0, 0), (10.0, 0)], rows, [1] * 60, prior)
    assert masked.posterior()[3, 2] == 0.0 and np.allclose(masked.posterior()[1, 1], 1.0)
    assert not hasattr(PR.OriginMaps, 'for_projection')


def test_log_weights_are_accepted_by_check_reweight():
    rows = np.array([[[-3.0, 2.0], [-1.0, 1.5]], [[-np.inf, 0.0], [-np.inf, 0.0]], [[-2.0, 4.0], [-np.inf, 0.0]]])
    om = _Stub(np.zeros((2, 3, 3)), np.ones((2, 3, 3)), 6, [(1.0, 0), (2.0, 0)], rows, [2, 1, 3])
    lw = om.log_weights()
    assert lw.shape == (6,) and lw[0] == lw[1] and lw[2] == -np.inf and lw[3] == lw[4] == lw[5]
    want0 = math.log((2.0 * math.exp(-3.0) + 1.5 * math.exp(-1.0)) / 2.0) - math.log(9.0)
    assert abs(lw[0] - want0) < 1e-14 and abs(lw[3] - (math.log(4.0 * math.exp(-2.0) / 2.0) - math.log(9.0))) < 1e-14
    plan = PR.check_reweight({'unknown origin': dict(log_weights=[lw])})
    assert plan['kinds'] == ['log_weights'] and np.array_equal(plan['log_weights'][0][0], lw)
    PR.check_reweight_rows(plan, [6])
    with np.errstate(divide='ignore'):
        prior = np.log(np.array([[0.5, 0.5, 0.0]] * 3))
    assert abs(PR.origin_log_prior_mass(prior, 9) - math.log(3.0)) < 1e-15


# ---------------------------------------------------------------- the restatement against its 40-digit version
def _small_case():
    N = 17
    fields = [{0: {d: OR.plume(N, 8 + 0.5 * d + 0.3 * m, 8 - 0.4 * d, 1.5 + 0.3 * d + 0.1 * m, 1.8 + 0.2 * d, 400.0)
                   for d in range(3)},
               1: {d: OR.plume(N, 8 + 0.7 * d, 8 + 0.2 * m, 1.4 + 0.4 * d, 1.6 + 0.1 * m, 400.0) for d in range(2)}}
              for m in range(5)]
    findings = [OR.probe(9, 7, 1, 'count', 0.5, 3), OR.probe(10, 9, 2, 'found', 0.25), OR.probe(0, 0, 1, 'none', 0.5),
                OR.probe(16, 16, 2, 'count', 0.5, 0), OR.probe(8, 8, 0, 'none', 0.02), OR.probe(7, 10, 2, 'count', 2.0, 1)]
    return N, fields, findings, [(0.5, 0), (2.0, 0), (1.0, 1)], [1, 3, 2, 1, 4]


@pytest.fixture(scope='module')
def small():
    N, fields, findings, hyp, weights = _small_case()
    ls = [OR.loglik(findings, hyp, f) for f in fields]
    mp = [OR.loglik_mp(findings, hyp, f) for f in fields]
    return types.SimpleNamespace(N=N, fields=fields, findings=findings, hyp=hyp, weights=weights, ls=ls, mp=mp)


def test_float64_restatement_against_mpmath(small):
    q = small
    O, M = len(q.findings), len(q.weights)
    worst = 0.0
    for l, (l_mp, parts) in zip(q.ls, q.mp):
        fin = OR.finite_mask(l_mp)
        assert np.array_equal(l != -np.inf, fin) and fin.any() and not fin.all()
        bound = OR.loglik_bound(O, parts)
        err = OR.diff(l[fin], l_mp[fin])
        assert (err <= bound[fin]).all()
        worst = max(worst, float((err / bound[fin]).max()))
    assert (q.ls[0][2] != -np.inf).sum() > 0                          # the lagged hypothesis is possible somewhere
    for f, (l_mp, parts) in zip(q.fields, q.mp):                     # the float64 parts are the mp version's
        assert np.allclose(OR.loglik_parts(q.findings, q.hyp, f), parts, rtol=1e-12, atol=0)
    A, S = OR.accumulate(q.ls, q.weights)
    E = OR.evidence(A, S, sum(q.weights))
    E_mp = OR.evidence_mp([l for l, _p in q.mp], q.weights)
    some = OR.finite_mask(E_mp)
    assert np.array_equal(E != -np.inf, some)
    lmax = np.max([OR.loglik_bound(O, p) for _l, p in q.mp], axis=0)
    err = OR.diff(E[some], E_mp[some])
    assert (err <= OR.evidence_bound(M, lmax, E)[some]).all()
    for l, (l_mp, parts) in zip(q.ls, q.mp):
        got, lb = OR.rows(l), OR.loglik_bound(O, parts)
        for h, (val, cells) in enumerate(OR.rows_mp(l_mp)):
            e = float(OR.diff([got[h, 0] + math.log(got[h, 1])], [val])[0])
            assert e <= OR.row_bound(float(lb[h].max()), cells, float(val))
    assert 0.0 < worst < 1.0


def test_merge_against_a_single_pass_and_another_order(small):
    q = small
    W, M, O = sum(q.weights), len(q.weights), len(q.findings)
    A, S = OR.accumulate(q.ls, q.weights)
    E = OR.evidence(A, S, W)
    A1, S1 = OR.accumulate(q.ls[:2], q.weights[:2])
    A2, S2 = OR.accumulate(q.ls[2:], q.weights[2:])
    Am, Sm = OR.merge(A1, S1, A2, S2)
    Ar, Sr = OR.accumulate(q.ls[::-1], q.weights[::-1])
    fin = E != -np.inf
    bound = (M + 8) * OR.EPS * (1.0 + np.abs(E))                     # the l are the same: only the update's own term
    for Ax, Sx in ((Am, Sm), (Ar, Sr)):
        assert np.array_equal(Ax, A)                                 # the maximum knows no order
        Ex = OR.evidence(Ax, Sx, W)
        assert np.array_equal(Ex != -np.inf, fin) and (np.abs(Ex[fin] - E[fin]) <= 2 * bound[fin]).all()
    assert np.array_equal(OR.merge(A, S, np.full_like(A, -np.inf), np.zeros_like(S))[1], S)      # -inf adds nothing
    a, s = OR.accumulate(q.ls, q.weights)
    assert np.array_equal(a, A) and np.array_equal(s, S)             # the same calls give the same bits


def test_twin_experiment_finds_the_known_origin():
    """8 synthetic Gaussian-plume members over 3 days at N = 65 (the numpy oracle of the chain); 4 counts rounded from
    member 3's field moved to a known origin 9 rows and -7 columns off the centre, 3 'none'.  The reference alone:
    regions of 3 and 9 cells, the mode on the known origin.  tests/test_origin_gpu.py runs the same inputs on the
    device."""
    members, findings = OR.twin_members(), OR.twin_findings()
    assert len(members) == 8 and [f['kind'] for f in findings] == ['count'] * 4 + ['none'] * 3
    assert all(f['n'] > 0 for f in findings[:4])
    ls = [OR.loglik(findings, OR.TWIN_HYP, m) for m in members]
    A, S = OR.accumulate(ls, OR.TWIN_WEIGHTS)
    P = PR.origin_posterior(PR.origin_log_evidence(A, S, sum(OR.TWIN_WEIGHTS)))[0]
    r50, r95 = PR.origin_region(P, 0.5), PR.origin_region(P, 0.95)
    assert r50[OR.TWIN_ORIGIN] == 1 and r95[OR.TWIN_ORIGIN] == 1
    assert (int(r50.sum()), int(r95.sum())) == (3, 9) and (r95 >= r50).all()
    mode = np.unravel_index(int(np.argmax(P)), P.shape)
    assert mode == OR.TWIN_ORIGIN
    assert P[32, 32] < 1e-6 * P.max()                    # "was it our release at the centre?": no


def test_shifted_read_as_a_slice_is_the_plain_one():
    rng = np.random.default_rng(3)
    for N in (7, 17):
        f = rng.random((N, N))
        for fr, fc in [(0, 0), (0, N - 1), (N - 1, 0), (N - 1, N - 1), (N // 2, N // 2), (2, N - 3)]:
            assert np.array_equal(OR.shifted(f, fr, fc), OR.shifted_plain(f, fr, fc))


def test_saved_block_where_no_cell_is_possible(tmp_path):
    """every E at -inf: the file is written with zero mass and empty regions, the block says why"""
    N = 5
    om = _Stub(np.full((1, N, N), -np.inf), np.zeros((1, N, N)), 3, [(1.0, 0)], [[[-np.inf, 0.0]]] * 2, [1, 2])
    om.plan = {'given': [[0.0, 0.0, 1, 'found', 1.0]]}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        path, block = PR.save_origin(str(tmp_path / 'pp'), om)
    assert 'no candidate cell' in block['impossible'] and block['masses'] is None and block['mode'] is None
    assert block['areas'] is None and block['diagnostics']['ess'] == 0.0 and block['members'] == 2
    f = np.load(path)
    assert (f['posterior'] == 0).all() and (f['region_l50'] == 0).all() and f['region_l95'].dtype == np.int8
    assert (f['log_evidence_h0'] == -np.inf).all() and f['member_rows'].shape == (2, 1, 2)


# ---------------------------------------------------------------- wiring
def test_driver_wiring_and_command_line():
    order = PR.FEED_ORDER['days']
    assert order.index('origin') == order.index('summary') + 1
    for kind in ('projection', 'sites', 'compare'):
        assert 'origin' not in PR.FEED_ORDER[kind]
    assert 'origin' in PR.ACCUMULATORS and PR.BUILD['origin'] is PR._build_origin and 'origin' in PR.FEED
    fs = PR._FieldSet().fed_from('days', object(), owns=False)
    assert PR.BUILD['origin'](fs, types.SimpleNamespace(or_plan=None)) is None and fs.origin is None
    assert PR.BUILD['origin'](fs, types.SimpleNamespace()) is None          # a request put together by hand
    q = types.SimpleNamespace(pop_model=None, chains=[], evaluate=lambda theta: None, origin=F1, days=None, thresholds=())
    with pytest.raises(ValueError, match='origin= needs the device: not with evaluate='):
        PR._check_request(q)
    src = open(os.path.join(ROOT, 'scripts', 'run_predictive.py')).read()
    for word in ('--origin', '--origin-amounts', '--origin-lags', '--origin-levels', '--origin-prior', 'origin_request',
                 "'%s_origin.npz' % args.out"):
        assert word in src, word
    lib = open(os.path.join(ROOT, 'parasitoids_amd', '_lib.py')).read()
    header = open(os.path.join(ROOT, 'include', 'parasitoid_hip.h')).read()
    for name in ('create', 'reserve', 'add', 'merge', 'reset', 'fetch', 'members', 'info', 'prof', 'destroy'):
        assert "'ps_origin_%s'" % name in lib and 'ps_origin_%s(' % name in header, name
    assert 'ps_origin.hip' in open(os.path.join(ROOT, 'parasitoids_amd', 'csrc', 'Makefile')).read()


# ---------------------------------------------------------------- the host emulation under the sanitizers
def _emulator(tmp_path, flags, name):
    exe = str(tmp_path / name)
    src = os.path.join(ROOT, 'tests', 'host', 'origin_emul.cpp')
    built = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-pthread'] + flags + ['-o', exe, src],
                           capture_output=True, text=True)
    return exe, built


def test_host_emulation_under_address_and_ub_sanitizers(tmp_path):
    """the shifted reads, the findings' order, the groups' order, the streaming pair and both stages of the member
    rows in the device's layout, on 8 threads, findings in all four corners, at N = 63, 64, 65 and 130, against a
    brute force.  Built with the address and the undefined-behaviour sanitizer; a child process."""
    exe, built = _emulator(tmp_path, ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined'], 'emul_asan')
    assert built.returncode == 0, built.stderr[-2000:]
    out = subprocess.run([exe, '63', '64', '65', '130'], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith('ok '), (out.stdout[-2000:], out.stderr[-2000:])
    assert int(out.stdout.split()[1]) == 5 + 2 * 4       # the group orders and the pair, two members per size


def test_host_emulation_under_the_thread_sanitizer(tmp_path):
    """the same program built with -fsanitize=thread, where this compiler links it and its runtime starts"""
    exe, built = _emulator(tmp_path, ['-fsanitize=thread'], 'emul_tsan')
    if built.returncode != 0:
        pytest.skip('this compiler does not link -fsanitize=thread')
    out = subprocess.run([exe, '63', '64', '65', '130'], capture_output=True, text=True)
    if out.returncode != 0 and 'FATAL: ThreadSanitizer' in out.stderr and 'FAIL' not in out.stdout:
        pytest.skip('the thread sanitizer does not start here: %s' % out.stderr.strip().splitlines()[0])
    assert out.returncode == 0 and out.stdout.startswith('ok '), (out.stdout[-2000:], out.stderr[-2000:])
