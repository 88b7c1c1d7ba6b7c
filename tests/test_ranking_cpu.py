"""CPU tests of the ranking of several named plans (predictive.PlanRanking): the numpy reference (rank_ref)
against an independent per-cell loop on small fields with planted ties, zeros and values at a threshold;
coverage_ranking against brute force; every refusal of ranking= that needs no device, in its stated order; and
the declared entry points."""
import itertools
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import contrast_ref
import rank_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = [1, 3, 1, 2, 1, 4]
THR = [0.5, 4.0]
SHAPE = (9, 9)


def _fields(seed, nplan):
    """[member][plan] random sparse fields, mostly zeros and the rest over four decades, with, in every member:
    cell (0, 0) zero for every plan; cell (0, 1) an exact positive tie of the plans 0 and 1 on top; cell (0, 2) an
    exact tie of all plans; cell (0, 3) plan 0 exactly at THR[0] and the others below; cell (0, 4) every plan exactly
    at THR[1]; cell (0, 5) the last plan alone on top"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in WEIGHTS:
        member = []
        for j in range(nplan):
            f = 10.0 ** rng.uniform(-2, 2, size=SHAPE)
            f[rng.random(SHAPE) < 0.6] = 0.0
            f[0, 0] = 0.0
            f[0, 1] = 7.25 if j < 2 else 0.125 * j
            f[0, 2] = 3.0
            f[0, 3] = THR[0] if j == 0 else 0.25
            f[0, 4] = THR[1]
            f[0, 5] = 50.0 if j == nplan - 1 else 1.0 + j
            member.append(f)
        out.append(member)
    return out


def _by_cell(fields, weights, thr, nplan):
    """the definitions, cell by cell in plain Python floats"""
    nk = len(thr)
    mean = np.zeros((nplan,) + SHAPE)
    m2 = np.zeros((nplan,) + SHAPE)
    best = np.zeros((nplan,) + SHAPE, dtype=np.int64)
    sole = np.zeros((nk, nplan) + SHAPE, dtype=np.int64)
    some = np.zeros((nk,) + SHAPE, dtype=np.int64)
    every = np.zeros((nk,) + SHAPE, dtype=np.int64)
    cells = []
    W = 0
    for member, w in zip(fields, weights):
        Wn = W + w
        row = [[0] * nk for _ in range(nplan)]
        for r, c in itertools.product(range(SHAPE[0]), range(SHAPE[1])):
            a = [float(member[j][r, c]) for j in range(nplan)]
            top = max(a)
            holders = [j for j in range(nplan) if a[j] == top]
            if len(holders) == 1:
                best[holders[0], r, c] += w
            for j in range(nplan):
                reg = top - a[j]
                d = reg - float(mean[j, r, c])
                if d != 0.0:
                    t = d * float(w)
                    new = float(mean[j, r, c]) + t / float(Wn)
                    wd = float(w) * d
                    m2[j, r, c] = float(m2[j, r, c]) + wd * (reg - new)
                    mean[j, r, c] = new
            for k, t in enumerate(thr):
                over = [j for j in range(nplan) if a[j] >= t]
                for j in over:
                    row[j][k] += 1
                if len(over) == 1:
                    sole[k, over[0], r, c] += w
                if over:
                    some[k, r, c] += w
                if len(over) == nplan:
                    every[k, r, c] += w
        cells.append(row)
        W = Wn
    return dict(mean=mean, M2=m2, best=best, sole=sole, any=some, all=every, cells=cells, W=W)


@pytest.mark.parametrize('nplan', [2, 3, 8])
def test_the_reference_against_a_loop_over_the_cells(nplan):
    fields = _fields(10 + nplan, nplan)
    st = rank_ref.new_state(SHAPE, nplan, THR)
    for member, w in zip(fields, WEIGHTS):
        rank_ref.add(st, member, w)
    want = _by_cell(fields, WEIGHTS, THR, nplan)
    W = sum(WEIGHTS)
    assert st['W'] == want['W'] == W and st['weights'] == WEIGHTS and st['cells'] == want['cells']
    for key in ('mean', 'M2', 'best', 'sole', 'any', 'all'):
        assert np.array_equal(st[key], want[key]), key
    # the planted cells: zeros and ties are nobody's, regret 0 for everyone on an all-plan tie
    assert not st['best'][:, 0, 0].any() and not st['best'][:, 0, 1].any() and not st['best'][:, 0, 2].any()
    assert not st['mean'][:, 0, 2].any() and not st['M2'][:, 0, 2].any() and not st['mean'][:, 0, 0].any()
    assert st['best'][nplan - 1, 0, 5] == W and not st['best'][:nplan - 1, 0, 5].any()
    assert st['mean'][0, 0, 1] == 0.0 and (nplan == 2 or st['mean'][2, 0, 1] == 7.25 - 0.25)
    assert st['sole'][0, 0, 0, 3] == W and not st['sole'][0, 1:, 0, 3].any()       # a value at the threshold reaches it
    assert st['any'][0, 0, 3] == W and st['all'][0, 0, 3] == 0
    assert st['all'][1, 0, 4] == W and st['any'][1, 0, 4] == W and not st['sole'][1, :, 0, 4].any()
    assert not st['any'][:, 0, 0].any()
    assert (st['all'] <= st['any']).all() and (st['all'] != st['any']).any()
    assert (st['best'].sum(axis=0) <= W).all() and (st['sole'].sum(axis=1) <= st['any']).all()
    # the device's order of the planes, and the rows
    planes = rank_ref.planes(st)
    assert len(planes) == nplan + len(THR) * (nplan + 2)
    assert planes[nplan - 1] is not None and np.array_equal(planes[nplan - 1], st['best'][nplan - 1])
    assert np.array_equal(planes[nplan + 1 * (nplan + 2) + 1], st['sole'][1, 1])
    assert np.array_equal(planes[nplan + nplan], st['any'][0]) and np.array_equal(planes[-1], st['all'][1])
    rows = rank_ref.rows(st)
    assert rows.shape == (len(WEIGHTS), nplan, len(THR))
    for i, member in enumerate(fields):
        for j in range(nplan):
            assert list(rows[i, j]) == [int((member[j] >= t).sum()) for t in THR]
    # against the plain definitions of the moments
    reg = rank_ref.regrets(fields)
    assert reg.min() == 0.0
    for j in range(nplan):
        mean, var = rank_ref.two_pass(reg[:, j], WEIGHTS)
        scale = reg[:, j].max()
        np.testing.assert_allclose(st['mean'][j], mean, rtol=1e-12, atol=1e-15 * scale)
        np.testing.assert_allclose(st['M2'][j] / W, var, rtol=1e-12, atol=1e-15 * scale ** 2)


def test_two_plans_are_the_contrast():
    fields = _fields(5, 2)
    st = rank_ref.new_state(SHAPE, 2, THR)
    con = contrast_ref.new_state(SHAPE, THR)
    for member, w in zip(fields, WEIGHTS):
        rank_ref.add(st, member, w)
        contrast_ref.add(con, member[0], member[1], w)
    assert np.array_equal(st['best'][0], con['pos']) and np.array_equal(st['best'][1], con['neg'])
    assert con['pos'].max() > 0 and con['neg'].max() > 0
    for k in range(len(THR)):
        assert np.array_equal(st['sole'][k, 0], con['gain'][k]) and np.array_equal(st['sole'][k, 1], con['loss'][k])
    assert [r[0] for r in st['cells']] == con['cells_a'] and [r[1] for r in st['cells']] == con['cells_b']


def test_permuting_the_plans_permutes_the_planes():
    fields = _fields(6, 3)
    perm = [2, 0, 1]
    a = rank_ref.new_state(SHAPE, 3, THR)
    b = rank_ref.new_state(SHAPE, 3, THR)
    for member, w in zip(fields, WEIGHTS):
        rank_ref.add(a, member, w)
        rank_ref.add(b, [member[j] for j in perm], w)
    for i, j in enumerate(perm):
        for key in ('mean', 'M2', 'best'):
            assert np.array_equal(b[key][i], a[key][j]), key
        assert np.array_equal(b['sole'][:, i], a['sole'][:, j])
    assert np.array_equal(b['any'], a['any']) and np.array_equal(b['all'], a['all'])


def _brute_ranking(cells, weights, area, levels):
    from parasitoids_amd.predictive import weighted_lower_quantile
    cells = np.asarray(cells)
    members, nplan, nout = cells.shape
    W = sum(weights)
    out = []
    for s in range(nout):
        plans = [dict(area=0, most=0, rank2=0, short=0) for _ in range(nplan)]
        tied = 0
        for i in range(members):
            x = [int(v) for v in cells[i, :, s]]
            top = max(x)
            if x.count(top) > 1:
                tied += weights[i]
            order = sorted(range(nplan), key=lambda j: -x[j])
            for j in range(nplan):
                same = [pos + 1 for pos, o in enumerate(order) if x[o] == x[j]]       # the ranks the tied plans share
                plans[j]['rank2'] += weights[i] * (2 * sum(same)) // len(same)
                plans[j]['area'] += weights[i] * x[j]
                plans[j]['short'] += weights[i] * (top - x[j])
                if x[j] == top and x.count(top) == 1:
                    plans[j]['most'] += weights[i]
        out.append({'plans': [{'mean': float(p['area']) / float(W) * area,
                               'quantiles': [float(weighted_lower_quantile(cells[:, j, s], np.array(weights), q)) * area
                                             for q in levels],
                               'p_most': float(p['most']) / float(W), 'mean_rank': float(p['rank2']) / float(2 * W),
                               'mean_shortfall': float(p['short']) / float(W) * area}
                              for j, p in enumerate(plans)],
                    'p_tied': float(tied) / float(W)})
    return out


def test_coverage_ranking_against_brute_force_and_by_hand():
    from parasitoids_amd.predictive import coverage_difference, coverage_ranking
    # three plans, four members, two outputs; output 0: a tie for the largest area in the members 0 and 3 (all three
    # in member 3), output 1: the order 2 > 1 > 0 throughout
    cells = np.array([[[5, 1], [5, 2], [3, 3]], [[1, 4], [4, 6], [2, 9]], [[7, 0], [2, 1], [2, 5]], [[6, 2], [6, 3], [6, 4]]])
    w = [2, 1, 3, 2]
    levels = (0.25, 0.5, 1.0)
    out = coverage_ranking(cells, w, 100.0, levels)
    assert out == _brute_ranking(cells, w, 100.0, levels)
    assert len(out) == 2 and set(out[0]) == {'plans', 'p_tied'} and len(out[0]['plans']) == 3
    assert set(out[0]['plans'][0]) == {'mean', 'quantiles', 'p_most', 'mean_rank', 'mean_shortfall'}
    p0, p1, p2 = out[0]['plans']
    assert out[0]['p_tied'] == 4.0 / 8.0                       # the members 0 and 3
    assert p0['p_most'] == 3.0 / 8.0 and p1['p_most'] == 1.0 / 8.0 and p2['p_most'] == 0.0
    # mid-ranks of plan 0: 1.5 (w 2), 3 (w 1), 1 (w 3), 2 (w 2) -> 13 / 8; of plan 2: 3, 2, 2.5, 2 -> 19.5 / 8
    assert p0['mean_rank'] == 13.0 / 8.0 and p2['mean_rank'] == 19.5 / 8.0
    assert p0['mean_rank'] + p1['mean_rank'] + p2['mean_rank'] == 6.0          # 1 + 2 + 3 in every member
    assert p0['mean'] == (10 + 1 + 21 + 12) / 8.0 * 100.0 and p0['mean_shortfall'] == 3.0 / 8.0 * 100.0
    assert p2['mean_shortfall'] == (4 + 2 + 15 + 0) / 8.0 * 100.0
    # areas of plan 0 sorted: 1 (w 1), 5 (w 2), 6 (w 2), 7 (w 3): cumulative 1, 3, 5, 8 against 2, 4, 8
    assert p0['quantiles'] == [500.0, 600.0, 700.0]
    assert out[1]['p_tied'] == 0.0 and [p['p_most'] for p in out[1]['plans']] == [0.0, 0.0, 1.0]
    assert [p['mean_rank'] for p in out[1]['plans']] == [3.0, 2.0, 1.0] and out[1]['plans'][2]['mean_shortfall'] == 0.0
    # random counts with many ties, eight plans
    rng = np.random.default_rng(3)
    big = rng.integers(0, 4, size=(17, 8, 3))
    bw = [int(v) for v in rng.integers(1, 5, size=17)]
    assert coverage_ranking(big, bw, 2.5) == _brute_ranking(big, bw, 2.5, (0.05, 0.5, 0.95))
    assert max(r['p_tied'] for r in coverage_ranking(big, bw, 2.5)) > 0
    # two plans: the shares of coverage_difference
    two = coverage_ranking(cells[:, :2], w, 100.0, levels)
    diff = coverage_difference(cells[:, 0], cells[:, 1], w, 100.0, levels)
    for r, d in zip(two, diff):
        assert r['plans'][0]['p_most'] == d['p_a_larger'] and r['plans'][1]['p_most'] == d['p_b_larger']
        assert r['p_tied'] == 1.0 - d['p_a_larger'] - d['p_b_larger']
        assert r['plans'][0]['mean'] - r['plans'][1]['mean'] == pytest.approx(d['mean'], rel=1e-14)
    # a member of weight 0 changes nothing
    again = coverage_ranking(np.concatenate([cells, [[[99, 0], [0, 99], [1, 1]]]]), w + [0], 100.0, levels)
    assert again == out
    with pytest.raises(ValueError, match='nothing accumulated'):
        coverage_ranking(cells, [0, 0, 0, 0], 100.0)
    with pytest.raises(ValueError, match='nothing accumulated'):
        coverage_ranking(np.zeros((0, 3, 2)), [], 100.0)
    with pytest.raises(ValueError, match='cell counts'):
        coverage_ranking(cells, w[:3], 100.0)
    with pytest.raises(ValueError, match='cell counts'):
        coverage_ranking(cells[:, 0], w, 100.0)
    with pytest.raises(ValueError):
        coverage_ranking(cells, w, 100.0, levels=(0.0,))


def _model(ndays=6, R=64):
    """what the checks read of a PopModel"""
    return types.SimpleNamespace(rad_dist=10000.0, rad_res=R, days=list(range(100, 100 + ndays)), r_number=130000,
                                 prob_model=False, device=None)


def test_the_ranking_argument_of_posterior_predictive():
    from parasitoids_amd.predictive import ranking_plan
    plan_a = dict(sites=[(0, 0, 0.6), (2000, 0, 0.4)], days=[0, 2, 5])
    b, c = dict(sites=[(0, 0, 1.0), (0, -2000, 0.5, 4)]), dict(sites=[(0, 0, 1.5)])
    rk = ranking_plan(dict(plans=[b, c], names=['now', 'late', 'one'], levels=(0.5,)), plan_a, _model())
    assert rk['names'] == ['now', 'late', 'one'] and rk['levels'] == [0.5] and len(rk['plans']) == 2
    sites, days, lags = rk['plans'][0]
    assert days == [0, 2, 5] and lags == [0, 4] and [s['drow'] for s in sites] == [0, 13]      # plan A's days
    assert rk['plans'][1][1] == [0, 2, 5] and rk['plans'][1][2] == [0]
    bare = ranking_plan([b, c], plan_a, _model())                                                 # the shorthand
    assert bare['plans'] == rk['plans'] and bare['names'] == ['plan0', 'plan1', 'plan2']
    assert bare['levels'] == [0.05, 0.5, 0.95]
    assert ranking_plan([c], dict(sites=[(0, 0, 2)]))['plans'][0][1] is None                      # no model yet
    assert ranking_plan([c], dict(sites=[(0, 0, 2)]), _model())['plans'][0][1] == list(range(6))
    assert len(ranking_plan([c] * 7, plan_a, _model())['plans']) == 7
    for bad, a, match in ((dict(sites=[(0, 0, 1)]), plan_a, 'ranking must be dict'),
                          (dict(plans=[c], days=[0, 1]), plan_a, 'ranking must be dict'),
                          (dict(plans=c), plan_a, 'ranking must be dict'),
                          (3.0, plan_a, 'ranking must be dict'),
                          ([c], None, 'give sites= too'),
                          ([], plan_a, '0 further plans'),
                          ([c] * 8, plan_a, '8 further plans; 1..7'),
                          ([c, dict(sites=[(0, 0, 1)], days=[0, 1])], plan_a, 'plan 2 must be dict.*output days'),
                          ([[(0, 0, 1)]], plan_a, 'plan 1 must be dict'),
                          (dict(plans=[c], names=['a']), plan_a, 'names must be 2'),
                          (dict(plans=[c], names='ab'), plan_a, 'names must be 2'),
                          (dict(plans=[c], names=['a', 'a']), plan_a, 'listed twice'),
                          (dict(plans=[c], levels=(0.0,)), plan_a, 'level|quantile'),
                          ([c], dict(sites=[]), 'release sites'),
                          ([c, dict(sites=[(0, 0, -1.0)])], plan_a, 'ranking: plan 2: .*amount'),
                          ([dict(sites=[(0, 0, 1, 1)])], plan_a, 'plan 1: .*smallest lag'),
                          ([dict(sites=[(0, 0, 1), (0, 0, 1, 6)])], plan_a, "beyond the model's 6 days"),
                          ([dict(sites=[(0, 0, 1), (0, 0, 1, 3)])], dict(sites=[(0, 0, 1)], days=[0, 2]),
                           'beyond the last output day'),
                          ([dict(sites=[(20200.0, 0, 1)])], plan_a, 'beyond the 129 x 129 domain')):
        with pytest.raises(ValueError, match=match):
            ranking_plan(bad, a, _model())
    # of two bad things the earlier in the stated order is reported: shape, sites=, the number of plans, a plan's
    # shape, names, levels, plan A, the further plans
    bad_plan, bad_sites = dict(sites=[(0, 0, 1)], days=[0]), dict(sites=[(0, 0, -1.0)])
    for bad, a, match in ((dict(plans=[c], extra=1), None, 'ranking must be dict'),
                          ([c] * 8, None, 'give sites= too'),
                          ([bad_plan] * 8, plan_a, '8 further plans'),
                          (dict(plans=[bad_plan], names=['a']), plan_a, 'plan 1 must be dict'),
                          (dict(plans=[c], names=['a'], levels=(2.0,)), plan_a, 'names must be 2'),
                          (dict(plans=[bad_sites], levels=(2.0,)), dict(sites=[]), 'level|quantile'),
                          ([bad_sites], dict(sites=[]), '^(?!ranking: plan).*release sites'),
                          ([c, bad_sites], plan_a, 'ranking: plan 2')):
        with pytest.raises(ValueError, match=match):
            ranking_plan(bad, a, _model())


def test_posterior_predictive_refuses_a_bad_ranking_before_evaluating():
    from parasitoids_amd.predictive import posterior_predictive
    calls = []
    trace = np.zeros((3, 1))

    def evaluate(theta):
        calls.append(theta)
        return None
    good = dict(sites=[(0, 0, 1.0)])
    with pytest.raises(ValueError, match='give sites= too'):
        posterior_predictive(None, (trace, ['x']), evaluate=evaluate, ranking=[good])
    with pytest.raises(ValueError, match='give sites= too'):
        posterior_predictive(_model(), (trace, ['x']), evaluate=evaluate, ranking=dict(plans=[good]))
    for ranking in ([(0, 0, 1)], [dict(sites=[])], [dict(sites=[(0, 0, 0.0)])], [dict(sites=[(0, 0, 1)], days=[0])],
                    [good] * 8, dict(plans=[good], names=['only'])):
        with pytest.raises(ValueError, match='ranking must be|release sites|amount|must be dict|further plans|names must'):
            posterior_predictive(None, (trace, ['x']), evaluate=evaluate, sites=good, ranking=ranking)
    with pytest.raises(ValueError, match="beyond the model's 6 days"):
        posterior_predictive(_model(), (trace, ['x']), evaluate=evaluate, sites=good,
                             ranking=[dict(sites=[(0, 0, 1), (0, 0, 1, 7)])])
    # the run's thresholds become the ranking's: > 0, increasing, at most 4
    for thr in ((0.0,), (10.0, 1.0), (1.0, 2.0, 3.0, 4.0, 5.0)):
        with pytest.raises(ValueError, match='finite and > 0|strictly increasing|at most 4'):
            posterior_predictive(None, (trace, ['x']), evaluate=evaluate, sites=good, ranking=[good], thresholds=thr)
    # compare= is checked first
    with pytest.raises(ValueError, match='compare must be'):
        posterior_predictive(None, (trace, ['x']), evaluate=evaluate, sites=good, compare=[(0, 0, 1)], ranking=3.0)
    assert not calls


def test_the_plan_ranking_class_refuses_before_it_touches_the_device():
    from parasitoids_amd.predictive import PlanRanking
    with pytest.raises(ValueError, match='1 plans; 2..8'):
        PlanRanking([object()])
    with pytest.raises(ValueError, match='9 plans; 2..8'):
        PlanRanking([object()] * 9)
    with pytest.raises(ValueError, match='ReleaseSites only or Projection only'):
        PlanRanking([object(), object()])
    assert 'not a recommendation' in PlanRanking.leader.__doc__


def test_rank_sites_needs_sites_on_the_command_line():
    """refused by the argument parser, before the package is imported"""
    script = os.path.join(ROOT, 'scripts', 'run_predictive.py')
    r = subprocess.run([sys.executable, script, '--synthetic', '--rank-sites', '0,0,1.5', '--rank-sites', '0,500,1'],
                       capture_output=True, text=True)
    assert r.returncode == 2 and '--rank-sites' in r.stderr and '--sites' in r.stderr
    r = subprocess.run([sys.executable, script, '--synthetic', '--sites', '0,0,1', '--rank-names', 'a,b'],
                       capture_output=True, text=True)
    assert r.returncode == 2 and '--rank-names' in r.stderr
    r = subprocess.run([sys.executable, script, '--help'], capture_output=True, text=True)
    assert r.returncode == 0 and '--rank-sites' in r.stdout and '--rank-names' in r.stdout


def test_the_rank_entry_points_are_declared_and_bound():
    from parasitoids_amd import _lib
    names = {'ps_rank_' + n for n in ('create', 'add_sites', 'add_project', 'merge', 'info', 'fetch', 'fetch_counts',
                                      'fetch_coverage', 'reset', 'prof', 'destroy')}
    assert names <= set(_lib.SIGNATURES)
    header = open(os.path.join(ROOT, 'include', 'parasitoid_hip.h')).read()
    assert {n for n in _lib.SIGNATURES if n.startswith('ps_rank_')} == names
    lib = _lib.load()
    for n in names:
        assert n + '(' in header and hasattr(lib, n), n
    assert len(_lib.SIGNATURES['ps_rank_create'][1]) == 7 and len(_lib.SIGNATURES['ps_rank_fetch'][1]) == 5
