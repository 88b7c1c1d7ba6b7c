"""CPU tests of the origin maps over known releases in the background: check_origin's known= key with every new
refusal, the float64 restatement (origin_known_ref) of bg, l and l0 against its 40-digit version within the unchanged
bounds of DESIGN 7y, the identity l == l0, the twin experiment with our own release known -- and without, which pins
why the feature exists -- the host functions of the second-source summary, the driver's wiring and the command line,
and the host emulation (tests/host/origin_known_emul.cpp over csrc/ps_origin_core.h) under the sanitizers."""
import math
import os
import subprocess
import types

import numpy as np
import pytest

import origin_known_ref as KR
import origin_ref as OR
from parasitoids_amd import predictive as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 10000.0 / 32
F1 = [(2 * RES, 3 * RES, 3, 'count', 0.02, 2), (-4 * RES, RES, 4, 'found', 0.05), (0.0, 0.0, 1, 'none', 0.01)]


# ---------------------------------------------------------------- check_origin
def test_check_origin_accepts_known_releases():
    plan = PR.check_origin(dict(findings=F1, known=[(0, 0, 1.0)]), 10000.0, 32, 6)
    assert plan['known_lags'] == [0] and plan['known_groups'] == [0] and plan['model_lags'] == [0]
    assert plan['known'][0]['drow'] == 0 and plan['known'][0]['dcol'] == 0 and plan['known_given'] == [[0.0, 0.0, 1.0, 0]]
    plan = PR.check_origin(dict(findings=F1, lags=[0, 1], known=[(2 * RES, -3 * RES, 0.5, 2), (0, 0, 1.0), (RES, 0, 2, 2)]),
                           10000.0, 32, 6)
    assert plan['known_lags'] == [0, 2] and plan['known_groups'] == [1, 0, 1]
    assert [(k['drow'], k['dcol']) for k in plan['known']] == [(3, 2), (0, 0), (0, 1)]
    assert plan['lags'] == [0, 1] and plan['groups'] == [0, 1] and plan['model_lags'] == [0, 1, 2]
    # a known release after the last finding (day 4) is allowed: it contributes 0 and needs no model
    plan = PR.check_origin(dict(findings=F1, known=[(0, 0, 1.0), (0, 0, 1.0, 5)]), 10000.0, 32, 6)
    assert plan['known_lags'] == [0, 5] and plan['model_lags'] == [0]
    # 'sites' takes the run's plan where one is handed in
    plan = PR.check_origin(dict(findings=F1, known='sites'), 10000.0, 32, 6, sites=[(0, 0, 0.6), (RES, 0, 0.5, 2)])
    assert plan['known_given'] == [[0.0, 0.0, 0.6, 0], [RES, 0.0, 0.5, 2]]
    # without known= the plan is what it was
    plan = PR.check_origin(F1, 10000.0, 32, 6)
    assert plan['known'] is None and plan['known_lags'] == [] and plan['model_lags'] == plan['lags'] == [0]
    assert PR.parse_origin_known('0,0,1; 625,-312.5,0.5,2') == [(0.0, 0.0, 1.0), (625.0, -312.5, 0.5, 2)]
    assert PR.parse_origin_known(' sites ') == 'sites'
    req = PR.origin_request('0,0,1,none,0.5', '0.5,1', '', '', '', 10000.0, 32, '0,0,1;625,0,0.5,1')
    assert req == dict(findings=[(0.0, 0.0, 1, 'none', 0.5)], amounts=[0.5, 1.0], known=[(0.0, 0.0, 1.0), (625.0, 0.0, 0.5, 1)])
    req = PR.origin_request('0,0,1,none,0.5', known='sites', sites=[(0, 0, 1.0)])
    assert req == dict(findings=[(0.0, 0.0, 1, 'none', 0.5)], known='sites')      # the driver resolves the word


@pytest.mark.parametrize('known, word', [
    ([(0, 0, 1.0, g) for g in range(5)], '5 different lags [0, 1, 2, 3, 4]'),
    ([(0, 0, 1.0), (0, 0, 1.0, 6)], 'known release 1: a release 6 days after the first lies beyond'),
    ('sites', "known='sites'"),
    ('ours', "or 'sites'"),
    ([], 'known: 0 release'),
    ([(0, 0, 1.0)] * 33, 'known: 33 release'),
    ([(0, 0, 0.0)], 'known release 0: amount'),
    ([(0, 0, 1.0, 1)], 'smallest lag must be 0'),
    ([(0, 0, 1.0), (1e6, 0, 1.0)], 'known release 1: offset'),
    ([(0, 0)], 'known release 0'),
    ([(0, 0, 1.0, 0.5)], 'known release 0'),
])
def test_check_origin_refuses_known_releases(known, word):
    with pytest.raises(ValueError, match='origin') as e:
        PR.check_origin(dict(findings=F1, known=known), 10000.0, 32, 6)
    assert word in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        PR.parse_origin_known('1,2')


# ---------------------------------------------------------------- the restatement against its 40-digit version
def _small_case():
    N = 17
    fields = [{0: {d: OR.plume(N, 8 + 0.5 * d + 0.3 * m, 8 - 0.4 * d, 1.5 + 0.3 * d + 0.1 * m, 1.8 + 0.2 * d, 400.0)
                   for d in range(3)},
               1: {d: OR.plume(N, 8 + 0.7 * d, 8 + 0.2 * m, 1.4 + 0.4 * d, 1.6 + 0.1 * m, 400.0) for d in range(2)}}
              for m in range(3)]
    findings = [OR.probe(9, 7, 1, 'count', 0.5, 3), OR.probe(10, 9, 2, 'found', 0.25), OR.probe(0, 0, 1, 'none', 0.5),
                OR.probe(16, 16, 2, 'count', 0.5, 0), OR.probe(8, 8, 0, 'none', 0.02), OR.probe(7, 10, 2, 'count', 2.0, 1),
                OR.probe(0, 16, 0, 'found', 0.5)]
    knowns = [KR.known(0, 0, 1.0, 0), KR.known(2, -1, 0.5, 1), KR.known(3, -2, 0.25, 0)]
    return N, fields, findings, [(0.5, 0), (2.0, 0), (1.0, 1)], knowns


def test_float64_restatement_against_mpmath():
    N, fields, findings, hyp, knowns = _small_case()
    O = len(findings)
    worst, some_excluded, some_identity = 0.0, False, False
    for f in fields:
        bg = KR.background(findings, knowns, f)
        assert bg.shape == (O,) and (bg >= 0).all() and (bg > 0).any()
        assert bg[6] == 0.0                                          # far from every known release: it can exclude
        assert bg[4] == (0.02 * 1.0) * f[0][0][8, 8] + (0.02 * 0.25) * f[0][0][5, 10]    # day 0 precedes the lag-1 release
        l = KR.loglik(findings, hyp, f, bg)
        l_mp, parts = KR.loglik_mp(findings, hyp, f, bg)
        fin = OR.finite_mask(l_mp)
        assert np.array_equal(l != -np.inf, fin) and fin.any()       # the -inf pattern: exact
        some_excluded |= not fin.all()
        bound = OR.loglik_bound(O, parts)
        err = OR.diff(l[fin], l_mp[fin])
        assert (err <= bound[fin]).all()
        worst = max(worst, float((err / bound[fin]).max()))
        l0 = KR.null_row(findings, bg)
        l0_mp, p0 = KR.null_row_mp(findings, bg)
        assert (l0 == -np.inf) == (l0_mp is None)
        if l0_mp is not None:
            assert OR.diff([l0], [l0_mp])[0] <= OR.loglik_bound(O, p0)
        free = KR.untouched(findings, hyp, f)
        if free.any():                                               # the identity: bit for bit
            some_identity = True
            assert (l[free] == l0).all() if l0 != -np.inf else (l[free] == -np.inf).all()
    assert some_excluded and some_identity and 0.0 < worst < 1.0
    # without known releases the restatement is origin_ref's, bit for bit
    zero = np.zeros(O)
    assert np.array_equal(KR.loglik(findings, hyp, fields[0], zero), OR.loglik(findings, hyp, fields[0]))


# ---------------------------------------------------------------- the twin experiment
@pytest.fixture(scope='module')
def twin():
    members = OR.twin_members()
    out = types.SimpleNamespace(members=members, hyp=KR.twin_hypotheses())
    for name, second in (('both', True), ('ours', False)):
        findings = KR.twin_findings(second, members)
        bgs = [KR.background(findings, KR.TWIN_KNOWN, m) for m in members]
        ls = [KR.loglik(findings, out.hyp, m, bg) for m, bg in zip(members, bgs)]
        l0s = [KR.null_row(findings, bg) for bg in bgs]
        setattr(out, name, types.SimpleNamespace(findings=findings, ls=ls, l0s=l0s))
    return out


def test_twin_experiment_with_our_release_known(twin):
    """our release of amount 1 at the centre is a fact; a second source of amount 0.5 at origin_ref.TWIN_ORIGIN.  With
    our release in the background the inversion finds the second source and says that one is needed; with the findings
    regenerated from our release alone it says that none is"""
    q = twin.both
    assert [f['n'] for f in q.findings[:7]] == [20, 9, 6, 6, 1, 0, 0]
    P, lbf = KR.twin_summary(q.ls, q.l0s, OR.TWIN_WEIGHTS)
    h, row, col = (int(v) for v in np.unravel_index(int(np.argmax(P)), P.shape))
    assert (row, col) == OR.TWIN_ORIGIN and twin.hyp[h] == (0.5, 0)
    Pm = P.sum(axis=0)
    r50, r95 = PR.origin_region(Pm, 0.5), PR.origin_region(Pm, 0.95)
    assert r50[OR.TWIN_ORIGIN] == 1 and r95[OR.TWIN_ORIGIN] == 1
    assert (int(r50.sum()), int(r95.sum())) == (5, 16)
    assert lbf > 50 and abs(lbf - 122.9) < 0.1
    _P, lbf0 = KR.twin_summary(twin.ours.ls, twin.ours.l0s, OR.TWIN_WEIGHTS)
    assert abs(lbf0) < 1 and abs(lbf0 + 0.24) < 0.01
    s = PR.origin_second_source(lbf + 3.0, 3.0, 0.5)
    assert s['log_bayes_factor'] == lbf and s['probability'] > 1 - 1e-12
    assert 0.3 < PR.origin_second_source(lbf0, 0.0, 0.5)['probability'] < 0.5


def test_twin_experiment_without_known_misses_the_second_source(twin):
    """why the feature exists: today's inversion of the same findings, every trap's catch explained by one source alone"""
    ls = [OR.loglik(twin.both.findings, twin.hyp, m) for m in twin.members]
    A, S = OR.accumulate(ls, OR.TWIN_WEIGHTS)
    P = PR.origin_posterior(PR.origin_log_evidence(A, S, sum(OR.TWIN_WEIGHTS)))
    h, row, col = (int(v) for v in np.unravel_index(int(np.argmax(P)), P.shape))
    assert (row, col) != OR.TWIN_ORIGIN and ((row, col), twin.hyp[h]) == ((35, 26), (1.0, 0))
    assert P[:, OR.TWIN_ORIGIN[0], OR.TWIN_ORIGIN[1]].sum() < 0.02


# ---------------------------------------------------------------- the host functions through the class
class _Stub(PR.OriginMaps):
    """the host side of OriginMaps over planes and rows given by hand: no device, no library"""

    def __init__(self, A, S, hypotheses, rows, weights, null_rows=None, prior=None, known=True):
        self._A, self._S = np.asarray(A, dtype=np.float64), np.asarray(S, dtype=np.float64)
        self.pairs, self.log_prior, self.levels = hypotheses, prior, [0.5, 0.95]
        self.N = self._A.shape[-1]
        self.pm = types.SimpleNamespace(rad_dist=1000.0, rad_res=self.N // 2)
        self.cell_area = (1000.0 / (self.N // 2)) ** 2
        self._rows, self._weights, self._null = rows, weights, null_rows
        self.known = [KR.known(0, 0, 1.0)] if known else None
        self.findings = [OR.probe(1, 1, 0, 'none', 1.0)]
        self.plan = {'given': [[0.0, 0.0, 0, 'none', 1.0]], 'known_given': [[0.0, 0.0, 1.0, 0]]}

    total_weight = property(lambda self: float(sum(self._weights)))
    members = property(lambda self: len(self._weights))

    def plane(self, what, h):
        return {'A': self._A, 'S': self._S}[what][h]

    def member_rows(self):
        return np.asarray(self._rows, dtype=np.float64), np.asarray(self._weights, dtype=np.int64)

    def null_rows(self):
        self._need_known('null_rows')
        return np.asarray(self._null, dtype=np.float64)

    def background(self):
        self._need_known('background')
        return np.array([0.125]), float(self._null[-1])

    def close(self):
        pass


def _stub(known=True):
    N, W = 3, [1, 3]
    # two members, one hypothesis: l_m(s) by hand, the planes and rows that the device would hold
    l = np.log(np.array([[[0.2, 0.1, 0.1], [0.4, 0.1, 0.1], [0.0, 0.0, 0.0]],
                         [[0.1, 0.1, 0.1], [0.8, 0.1, 0.2], [0.0, 0.0, 0.1]]]) + 1e-300)
    l[l < -600] = -np.inf
    A, S = OR.accumulate([l[0][None], l[1][None]], W)
    rows = [OR.rows(l[m][None]) for m in range(2)]
    return _Stub(A, S, [(1.0, 0)], rows, W, [math.log(0.05), math.log(0.2)], known=known), l, W


def test_second_source_summary_through_the_class(tmp_path):
    om, l, W = _stub()
    null = math.log((1 * 0.05 + 3 * 0.2) / 4.0)
    second = math.log((1 * np.exp(l[0]).sum() + 3 * np.exp(l[1]).sum()) / 4.0 / 9.0)
    assert abs(om.log_evidence_null() - null) < 1e-14 and abs(om.log_evidence_second() - second) < 1e-14
    s = om.second_source()
    assert sorted(s) == sorted(['log_bayes_factor', 'probability', 'prior', 'log_evidence_second', 'log_evidence_null',
                                'ess_second', 'ess_null'])
    assert abs(s['log_bayes_factor'] - (second - null)) < 1e-14 and s['prior'] == 0.5
    bf = math.exp(second - null)
    assert abs(s['probability'] - bf / (1 + bf)) < 1e-14
    assert abs(om.second_source(prior=0.1)['probability'] - 0.1 * bf / (0.1 * bf + 0.9)) < 1e-14
    assert abs(s['ess_null'] - (0.05 + 3 * 0.2) ** 2 / (0.05 ** 2 + 3 * 0.2 ** 2)) < 1e-12 and 1.0 <= s['ess_second'] <= 4.0
    for bad in (-0.1, 1.5, 'x'):
        with pytest.raises(ValueError, match='prior probability'):
            om.second_source(prior=bad)
    # log_weights: None gives the rows as today, a number the mixture of both explanations per row
    lw = om.log_weights()
    assert lw.shape == (4,) and abs(lw[0] - math.log(np.exp(l[0]).sum() / 9.0)) < 1e-14
    mix = om.log_weights(prior_second=0.25)
    l0 = np.repeat(om.null_rows(), W)
    assert np.allclose(np.exp(mix), 0.25 * np.exp(lw) + 0.75 * np.exp(l0), rtol=1e-14, atol=0)
    assert np.array_equal(om.log_weights(prior_second=1.0), lw) and np.allclose(om.log_weights(prior_second=0.0), l0)
    # the files: the new keys only where known was given
    path, block = PR.save_origin(str(tmp_path / 'k'), om)
    f = np.load(path)
    assert {'known', 'null_rows', 'background_last'} <= set(f.files) and f['known'].tolist() == [[0.0, 0.0, 1.0, 0.0]]
    assert np.array_equal(f['null_rows'], om.null_rows()) and f['background_last'].tolist() == [0.125]
    assert block['second_source'] == om.second_source() and block['known'] == [[0.0, 0.0, 1.0, 0]]
    plain, _l, _W = _stub(known=False)
    path, block = PR.save_origin(str(tmp_path / 'p'), plain)
    assert not {'known', 'null_rows', 'background_last'} & set(np.load(path).files)
    assert 'second_source' not in block and 'known' not in block
    assert np.array_equal(plain.log_weights(), lw)
    for name in ('background', 'null_rows', 'log_evidence_null', 'log_evidence_second', 'second_source'):
        with pytest.raises(ValueError, match='no known releases'):
            getattr(plain, name)()
    with pytest.raises(ValueError, match='no known releases'):
        plain.log_weights(prior_second=0.5)


# ---------------------------------------------------------------- wiring
def test_driver_wiring_and_command_line():
    src = open(os.path.join(ROOT, 'scripts', 'run_predictive.py')).read()
    for word in ('--origin-known', 'args.origin_known', "sites['sites'] if sites else None"):
        assert word in src, word
    lib = open(os.path.join(ROOT, 'parasitoids_amd', '_lib.py')).read()
    header = open(os.path.join(ROOT, 'include', 'parasitoid_hip.h')).read()
    for name in ('set_known', 'background', 'fetch_background', 'null_rows'):
        assert "'ps_origin_%s'" % name in lib and 'ps_origin_%s(' % name in header, name
    # the definitions stand in the header in the order of the issue
    at = [header.index(w) for w in ('known releases  k = 0', 'background per member', 'likelihood for candidate',
                                    'null row   per member', 'identity   at a candidate')]
    assert at == sorted(at)
    # the driver's request: known='sites' takes the plan's sites, and is refused by name without a plan
    common = dict(pop_model=None, chains=[], evaluate=None, days=None, thresholds=())
    q = types.SimpleNamespace(origin=dict(findings=F1, known='sites'), sites=None, **common)
    with pytest.raises(ValueError, match="known='sites'"):
        PR._check_request(q)
    # the command line's request round-trips
    text = ';'.join(','.join(str(x) for x in f) for f in F1)
    req = PR.origin_request(text, '0.25,0.5,1', '', '', '', 10000.0, 32, '0.0,0.0,1.0;312.5,-625.0,0.5,2')
    assert req == dict(findings=[tuple(f) for f in F1], amounts=[0.25, 0.5, 1.0],
                       known=[(0.0, 0.0, 1.0), (312.5, -625.0, 0.5, 2)])
    plan = PR.check_origin(req, 10000.0, 32, 6)
    assert plan['known_given'] == [[0.0, 0.0, 1.0, 0], [312.5, -625.0, 0.5, 2]] and plan['model_lags'] == [0, 2]


# ---------------------------------------------------------------- the host emulation under the sanitizers
def _emulator(tmp_path, flags, name):
    exe = str(tmp_path / name)
    src = os.path.join(ROOT, 'tests', 'host', 'origin_known_emul.cpp')
    built = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-pthread'] + flags + ['-o', exe, src],
                           capture_output=True, text=True)
    return exe, built


def test_host_emulation_under_the_sanitizers(tmp_path):
    """the background's index arithmetic at the domain's edges, the sum across the known groups in index order, the
    null row's order, the identity and the order of a member's calls, at N = 63, 64, 65 and 130: a stand-alone program
    built with the address and the undefined-behaviour sanitizer, run as a child process; once more with the thread
    sanitizer where this compiler links it and its runtime starts"""
    exe, built = _emulator(tmp_path, ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined'], 'kemul_asan')
    assert built.returncode == 0, built.stderr[-2000:]
    out = subprocess.run([exe, '63', '64', '65', '130'], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith('ok '), (out.stdout[-2000:], out.stderr[-2000:])
    assert int(out.stdout.split()[1]) == 16 + 4            # every (known groups, groups) pair, and the four sizes
    exe, built = _emulator(tmp_path, ['-fsanitize=thread'], 'kemul_tsan')
    if built.returncode == 0:
        out = subprocess.run([exe, '63', '64', '65', '130'], capture_output=True, text=True)
        started = not (out.returncode != 0 and 'FATAL: ThreadSanitizer' in out.stderr and 'FAIL' not in out.stdout)
        if started:
            assert out.returncode == 0 and out.stdout.startswith('ok '), (out.stdout[-2000:], out.stderr[-2000:])
