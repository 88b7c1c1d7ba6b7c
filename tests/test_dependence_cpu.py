"""Host-side tests of the dependence maps (predictive.DependenceMaps and its helpers): the bin edges, the numpy
replay (depend_ref) against the two-pass definition of the correlation ratio, the reason for the feature on
synthetic fields -- a dependence through an even function that the correlation does not see --, the argument
checks, the driver's tables, and the refusal of a finalize over too few members per bin."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import depend_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def _bins(edges, values):
    return np.searchsorted(edges, values, side='right')


def test_edges_equal_weight_and_midpoints():
    from parasitoids_amd.predictive import dependence_edges
    v = np.linspace(110.0, 250.0, 12)
    e = dependence_edges(v, np.ones(12, dtype=int), 4)
    assert e.tolist() == [(v[2] + v[3]) / 2, (v[5] + v[6]) / 2, (v[8] + v[9]) / 2]
    assert np.bincount(_bins(e, v)).tolist() == [3, 3, 3, 3]
    # the order of the members does not matter, and no value sits on an edge
    perm = np.random.default_rng(0).permutation(12)
    assert np.array_equal(dependence_edges(v[perm], np.ones(12, dtype=int), 4), e)
    assert not np.isin(e, v).any() and np.all(np.diff(e) > 0)
    e6 = dependence_edges(v, np.ones(12, dtype=int), 6)
    assert np.bincount(_bins(e6, v)).tolist() == [2] * 6


def test_edges_equal_values_share_a_bin():
    from parasitoids_amd.predictive import dependence_edges
    v = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 2.0, 3.0, 4.0])
    e = dependence_edges(v, np.ones(8, dtype=int), 4)
    # the quarter points fall inside the five equal values: they stay together, and the cuts that fall together
    # are one
    assert e.tolist() == [1.5, 2.5] and np.bincount(_bins(e, v)).tolist() == [5, 1, 2]
    b = _bins(e, v)
    assert len(set(b[:5])) == 1


def test_edges_are_decided_in_integers():
    from parasitoids_amd.predictive import dependence_edges
    # three values of weight 1/3 each in floating point would leave the half point to rounding; in integers
    # |c bins - j total| is 1 for both neighbours of the half, and the tie goes to the lower value
    v = np.array([0.1, 0.2, 0.3, 0.4])
    w = np.array([1, 1, 1, 3])
    e = dependence_edges(v, w, 2)               # cumulative 1, 2, 3 | 6: 2 c against 6 -> c = 3 exactly
    assert e.tolist() == [0.3 + 0.5 * (0.4 - 0.3)]
    w = np.array([2, 1, 1, 2])                  # cumulative 2, 3, 4 | 6: c = 3 exactly, behind the second value
    assert dependence_edges(v, w, 2).tolist() == [0.2 + 0.5 * (0.3 - 0.2)]
    w = np.array([2, 2, 2, 1])                  # cumulative 2, 4, 6 | 7: |4 - 7| = 3, |8 - 7| = 1, |12 - 7| = 5
    assert dependence_edges(v, w, 2).tolist() == [0.2 + 0.5 * (0.3 - 0.2)]
    w = np.array([1, 2, 2, 1])                  # cumulative 1, 3, 5 | 6: a tie between 3 and ... 2 c = 6 at c = 3
    assert dependence_edges(v, w, 2).tolist() == [0.2 + 0.5 * (0.3 - 0.2)]
    w = np.array([2, 2, 2, 2])                  # cumulative 2, 4, 6 | 8, three bins: 3 c against 8 and 16
    # |6 - 8| = 2, |12 - 8| = 4 -> behind the first; |12 - 16| = 4, |18 - 16| = 2 -> behind the third
    assert np.bincount(_bins(dependence_edges(v, w, 3), v)).tolist() == [1, 2, 1]
    # huge weights stay exact
    big = np.array([2 ** 31, 2 ** 31 - 1, 1, 2 ** 31], dtype=np.int64)
    assert np.bincount(_bins(dependence_edges(v, big, 2), v)).tolist() == [2, 2]


def test_edges_fewer_distinct_values_than_bins_and_a_constant():
    from parasitoids_amd.predictive import dependence_edges
    v = np.array([5.0, 7.0, 5.0, 9.0, 7.0, 5.0])
    e = dependence_edges(v, np.ones(6, dtype=int), 8)
    assert e.tolist() == [6.0, 8.0]             # three distinct values: three bins
    assert dependence_edges(np.full(9, 3.25), np.arange(1, 10), 8).size == 0
    # neighbouring doubles: the midpoint rounds onto one of them, the upper value still goes right
    lo = 1.0
    hi = np.nextafter(lo, 2.0)
    e = dependence_edges(np.array([lo, hi]), np.array([1, 1]), 2)
    assert e.size == 1 and _bins(e, np.array([lo, hi])).tolist() == [0, 1]
    for bad in (1, 17, 2.5):
        with pytest.raises(ValueError, match='bins'):
            dependence_edges(v, np.ones(6, dtype=int), bad)
    with pytest.raises(ValueError, match='positive integers'):
        dependence_edges(v, np.array([1, 1, 0, 1, 1, 1]), 2)
    with pytest.raises(ValueError, match='finite'):
        dependence_edges(np.array([1.0, np.nan]), np.array([1, 1]), 2)


def test_edges_with_run_lengths_as_weights():
    from parasitoids_amd.predictive import dependence_edges
    # a chain's runs: the value of a run counts with its length, as if every row were listed
    v = np.array([3.0, 1.0, 2.0, 5.0, 4.0])
    n = np.array([4, 1, 2, 1, 2])
    rows = np.repeat(v, n)
    for bins in (2, 3, 4, 5):
        assert np.array_equal(dependence_edges(v, n, bins), dependence_edges(rows, np.ones(rows.size, dtype=int), bins))
    e = dependence_edges(v, n, 2)               # cumulative by value 1, 3, 7, 9 | 10: 2 c nearest 10 -> c = 3 or 7
    assert e.tolist() == [2.5]                  # the tie goes to the lower value


def _replay(fields, bins, weights, nbin):
    nparam = bins.shape[1]
    st = depend_ref.new_state(fields.shape[1:], nparam, nbin)
    for f, b, w in zip(fields, bins, weights):
        depend_ref.add(st, f, b, w)
    W = float(st['W'])
    eta, dom = depend_ref.finalize(st['mean'], st['M2'] / W, st['S'], st['Wb'])
    return st, eta, dom


def test_replay_matches_the_two_pass_definition():
    """The tolerance, relative to the field scale X = max |v| and not tuned: with n members and B bins a bin sum
    carries at most n_b + 1 roundings, (n_b + 1) u W_b X; the Welford mean about 3 n u X; so a bin mean minus the
    mean is off by at most (4 n + 3) u X, its square -- |d| <= 2 X -- by 4 X (4 n + 3) u X + 4 u X^2, and the
    weighted average over the bins adds B + 2 roundings of at most 4 X^2: the between-bin variance is off by at most
    (16 n + 4 B + 24) u X^2.  M2 / W carries the mean's error in both factors of w d (v - mean'), 12 n u X^2, four
    roundings of at most 4 X^2 and the n roundings of the sum: (13 n + 16) u X^2.  With eta <= 1,
    |eta - eta_ref| var <= (29 n + 4 B + 40) u X^2; the two-pass reference is allowed as much again."""
    rng = np.random.default_rng(11)
    n, B, shape = 40, 4, (9, 7)
    fields = rng.gamma(2.0, 50.0, size=(n,) + shape)
    fields[:, 0, :] = 0.0                                # cells that never vary
    fields[::3, 1, :] = 0.0                              # and cells that are 0 in some members
    weights = rng.integers(1, 6, size=n)
    bins = np.stack([rng.integers(0, B, size=n), np.sort(rng.integers(0, B, size=n)), np.zeros(n, dtype=int)], axis=1)
    st, eta, dom = _replay(fields, bins, weights, B)
    X = np.abs(fields).max()
    tol = 2 * (29 * n + 4 * B + 40) * U * X ** 2
    for p in range(3):
        ref, mean, var = depend_ref.ratio(fields, bins[:, p], weights)
        assert np.abs(st['mean'] - mean).max() <= 3 * n * U * X * 2
        err = np.abs(eta[p] - ref) * var
        print('parameter %d: max |eta - two-pass| var = %.3g, allowed %.3g' % (p, err.max(), tol))
        assert err.max() <= tol
        assert eta[p].min() >= 0.0 and eta[p].max() <= 1.0
    assert not eta[2].any()                              # one bin: no between-bin variance at all
    assert not eta[:, 0, :].any() and np.all(dom[0, :] == -1)
    assert set(np.unique(dom[1:])) <= {0, 1}             # never the constant one
    # merging two halves: the bin sums are sums, the moments Chan's
    a = depend_ref.new_state(shape, 3, B)
    b = depend_ref.new_state(shape, 3, B)
    for i, (f, bb, w) in enumerate(zip(fields, bins, weights)):
        depend_ref.add(a if i < 17 else b, f, bb, w)
    keep = {k: np.copy(v) for k, v in b.items() if isinstance(v, np.ndarray)}
    depend_ref.merge(a, b)
    assert a['W'] == st['W'] and a['members'] == n and np.array_equal(a['Wb'], st['Wb'])
    np.testing.assert_allclose(a['S'], st['S'], rtol=0, atol=(n + 1) * U * X * st['W'])
    np.testing.assert_allclose(a['mean'], st['mean'], rtol=0, atol=6 * n * U * X)
    np.testing.assert_allclose(a['M2'] / a['W'], st['M2'] / st['W'], rtol=0, atol=2 * (13 * n + 16) * U * X ** 2)
    assert all(np.array_equal(b[k], v) for k, v in keep.items())      # the source stays as it is
    e = depend_ref.merge(depend_ref.new_state(shape, 3, B), st)
    assert all(np.array_equal(e[k], st[k]) for k in ('mean', 'M2', 'S', 'Wb')) and e['W'] == st['W']


def test_an_even_dependence_is_seen_by_the_ratio_and_not_by_the_correlation():
    """v = a(cell) theta^2 with theta symmetric about 0: the correlation with theta is 0, the cell depends on
    nothing else.  400 members, 8 bins: the within-bin variance of theta^2 over eight bins of [-1, 1] leaves
    eta^2 = 0.92; an unrelated parameter stays at its floor."""
    from parasitoids_amd.predictive import adjusted_ratio, dependence_edges
    n, B = 400, 8
    theta = np.linspace(-1.0, 1.0, n)
    other = np.random.default_rng(2024).normal(size=n)
    a = np.linspace(0.0, 3.0, 12).reshape(3, 4)
    fields = a[None] * (theta ** 2)[:, None, None]
    w = np.ones(n, dtype=int)
    edges = [dependence_edges(theta, w, B), dependence_edges(other, w, B)]
    assert all(e.size == B - 1 for e in edges)
    bins = np.stack([_bins(edges[0], theta), _bins(edges[1], other)], axis=1)
    assert np.bincount(bins[:, 0]).tolist() == [50] * B and np.bincount(bins[:, 1]).tolist() == [50] * B
    st, eta, dom = _replay(fields, bins, w, B)
    live = a > 0
    mean, var = fields.mean(0), fields.var(0)
    cov = ((theta - theta.mean())[:, None, None] * (fields - mean[None])).mean(0)
    r2 = np.zeros(a.shape)
    np.divide(cov ** 2, var * theta.var(), out=r2, where=live)
    print('r2 max %.3g, eta2 of theta min %.4f, of the unrelated one median %.4f (floor %.4f)'
          % (r2[live].max(), eta[0][live].min(), np.median(eta[1][live]), (B - 1) / (n - 1)))
    assert r2[live].max() < 0.05 and eta[0][live].min() > 0.9
    assert not eta[:, ~live].any() and np.all(dom[live] == 0) and np.all(dom[~live] == -1)
    adj = adjusted_ratio(eta[1], n, B)
    assert np.median(adj[live]) < 0.05
    # the adjustment takes the floor away and leaves a strong ratio nearly as it is
    assert adjusted_ratio((B - 1) / (n - 1), n, B) == pytest.approx(0.0, abs=1e-15)
    assert adjusted_ratio(0.0, n, B) == 0.0 and adjusted_ratio(1.0, n, B) == 1.0
    assert np.all(adjusted_ratio(eta[0], n, B)[live] > 0.9)
    with pytest.raises(ValueError, match='nothing is left'):
        adjusted_ratio(0.5, 8, 8)


def test_check_dependence_refusals():
    from parasitoids_amd import mcmc
    from parasitoids_amd.predictive import check_dependence
    names = [m[0] for m in mcmc.MODEL_BLOCK]
    assert check_dependence(True) == {'params': names, 'bins': 8, 'days': None}
    assert check_dependence(['sig_x', 'mu_r']) == {'params': ['sig_x', 'mu_r'], 'bins': 8, 'days': None}
    assert check_dependence('sig_x')['params'] == ['sig_x']
    got = check_dependence(dict(params=['sig_y'], bins=2, days=[0, 3]))
    assert got == {'params': ['sig_y'], 'bins': 2, 'days': [0, 3]}
    assert check_dependence(dict(bins=16))['params'] == names
    for bad in (1, 17, 0, -2, 2.5, '8', None, True):
        with pytest.raises(ValueError, match='bins'):
            check_dependence(dict(params=['sig_x'], bins=bad))
    with pytest.raises(ValueError, match='unknown sensitivity parameters'):
        check_dependence(['nothing'])
    with pytest.raises(ValueError, match='listed twice'):
        check_dependence(dict(params=['sig_x', 'sig_x']))
    with pytest.raises(ValueError, match='unknown keys'):
        check_dependence(dict(params=['sig_x'], bin=4))
    with pytest.raises(ValueError, match='True or a list'):
        check_dependence(dict(params=3))
    for bad in ([], [2, 1], [-1, 0], 'ab', 3):
        with pytest.raises(ValueError, match='days'):
            check_dependence(dict(params=['sig_x'], days=bad))


def test_the_driver_refuses_bad_arguments_before_any_evaluation():
    from parasitoids_amd import predictive as PR
    calls = []
    chain = (np.zeros((3, len(PR.model_names()))), PR.model_names())
    pm = types.SimpleNamespace(days=list(range(4)), rad_dist=8000.0, rad_res=8, device=None,
                               evaluate=lambda *a, **k: calls.append(a))
    with pytest.raises(ValueError, match='bins'):
        PR.posterior_predictive(pm, chain, dependence=dict(params=['sig_x'], bins=1))
    with pytest.raises(ValueError, match='unknown sensitivity parameters'):
        PR.posterior_predictive(pm, chain, dependence=['nope'])
    with pytest.raises(ValueError, match='day 4 is not among'):
        PR.posterior_predictive(pm, chain, dependence=dict(params=['sig_x'], days=[1, 4]))
    with pytest.raises(ValueError, match='not with evaluate='):
        PR.posterior_predictive(None, chain, evaluate=lambda theta: None, dependence=True)
    assert not calls


def test_without_dependence_nothing_is_built():
    from parasitoids_amd import predictive as PR
    for kind in ('days', 'projection', 'sites'):
        order = PR.FEED_ORDER[kind]
        assert order[order.index('sensitivity') + 1] == 'dependence', kind
    assert PR.FEED_ORDER['days'][-1] == 'modes' and PR.FEED_ORDER['sites'][-1] == 'modes'
    assert 'dependence' not in PR.FEED_ORDER['compare']
    assert 'dependence' in PR.ACCUMULATORS and 'dependence' in PR.BUILD and 'dependence' in PR.FEED
    q = types.SimpleNamespace(dp_plan=None, dp_edges=None)
    fs = PR._FieldSet().fed_from('days', object(), owns=False)
    assert PR.BUILD['dependence'](fs, q) is None and fs.dependence is None
    assert PR.ProjectedMaps(None, None, None, None).dependence is None
    # the request of a call without the argument carries no plan, and the result no maps
    chain = (np.zeros((3, len(PR.model_names()))), PR.model_names())
    res = PR.posterior_predictive(None, chain, evaluate=lambda theta: None)
    assert res.dependence is None
    # a member is fed the run's theta and length
    fed = []
    acc = types.SimpleNamespace(add=lambda theta, w: fed.append((theta, w)))
    PR.FEED['dependence'](acc, None, types.SimpleNamespace(theta='t', length=3))
    assert fed == [('t', 3)]


def test_a_handle_that_does_not_fit_is_a_value_error_that_names_the_gigabytes(monkeypatch):
    from parasitoids_amd import _lib as L
    from parasitoids_amd import predictive as PR

    class Full():
        def __init__(self, *args):
            raise L.HipError(L.PS_ERR_OOM, 'depend_create: 12.7 GB, 1 GB free')

        @classmethod
        def for_projection(cls, *args):
            raise L.HipError(L.PS_ERR_BAD_ARG, 'something else')
    monkeypatch.setattr(PR, 'DependenceMaps', Full)
    names = PR.model_names()
    q = types.SimpleNamespace(dp_plan=dict(params=names, bins=8, days=None), dp_edges=[np.arange(7.0)] * 15)
    fs = PR._FieldSet().fed_from('days', types.SimpleNamespace(rad_res=400), owns=False)
    fs._days = list(range(18))
    with pytest.raises(ValueError, match=r'15 parameters x 8 bins x 18 slots need 12\.7 GB.*days= and a shorter'):
        PR.BUILD['dependence'](fs, q)
    fs = PR._FieldSet().fed_from('projection', types.SimpleNamespace(pm=types.SimpleNamespace(rad_res=400), nout=2))
    with pytest.raises(L.HipError):                      # any other device error stays what it is
        PR.BUILD['dependence'](fs, q)


def test_pooled_edges_span_all_chains():
    from parasitoids_amd import predictive as PR
    names = PR.model_names()
    ix = names.index('sig_x')
    rows_a = np.zeros((5, len(names)))
    rows_b = np.zeros((4, len(names)))
    rows_a[:, ix] = [1.0, 1.0, 2.0, 3.0, 3.0]
    rows_b[:, ix] = [4.0, 5.0, 5.0, 6.0]
    cols = list(range(len(names)))
    prepared = [(rows_a, [(0, 2), (2, 1), (3, 2)], cols, None, 'a'), (rows_b, [(0, 1), (1, 2), (3, 1)], cols, None, 'b')]
    e_x, e_c = PR.pooled_dependence_edges(prepared, ['sig_x', 'mu_r'], 3)
    # nine rows: cumulative 2, 3, 5, 6, 8, 9 -> 3 c nearest 9 and 18: c = 3 and c = 6
    assert e_x.tolist() == [2.5, 4.5] and e_c.size == 0


def test_the_script_refuses_bad_names_and_bins_before_any_work():
    script = os.path.join(ROOT, 'scripts', 'run_predictive.py')
    for extra, word in ((['--dependence', 'sig_x', '--dependence-bins', '1'], 'bins must be an integer in 2..16'),
                        (['--dependence', 'sig_x', '--dependence-bins', '17'], 'bins must be an integer in 2..16'),
                        (['--dependence', 'nope'], 'unknown sensitivity parameters')):
        r = subprocess.run([sys.executable, script, '--synthetic'] + extra, capture_output=True, text=True)
        assert r.returncode != 0 and word in r.stderr and 'members_per_hour' not in r.stdout, (extra, r.stderr[-300:])
    src = open(script).read()
    for key in ('dependence_add_ms_per_member', 'dependence_bytes'):
        assert key in src


def test_the_dependence_entry_points_are_declared_and_bound():
    from parasitoids_amd import _lib
    names = {'ps_depend_' + n for n in ('create', 'add', 'add_project', 'add_sites', 'merge', 'finalize', 'fetch', 'info',
                                        'reset', 'prof', 'destroy')}
    assert names <= set(_lib.SIGNATURES)
    header = open(os.path.join(ROOT, 'include', 'parasitoid_hip.h')).read()
    lib = _lib.load()
    for n in names:
        assert n + '(' in header and hasattr(lib, n), n


def test_finalize_refuses_fewer_than_two_members_per_bin():
    from parasitoids_amd.predictive import finalize_bin_weights
    Wb = np.array([[2, 1, 2, 0], [5, 0, 0, 0]])
    out = finalize_bin_weights(['sig_x', 'mu_r'], Wb, 6)          # three bins used, six members
    assert out.dtype == np.float64 and out.flags['C_CONTIGUOUS'] and np.array_equal(out, Wb)
    with pytest.raises(ValueError, match="5 members in 3 bins of 'sig_x'"):
        finalize_bin_weights(['sig_x', 'mu_r'], Wb, 5)
    finalize_bin_weights(['mu_r'], Wb[1:], 2)                     # a constant parameter: one bin, two members
    with pytest.raises(ValueError, match="1 members in 1 bins of 'mu_r'"):
        finalize_bin_weights(['mu_r'], Wb[1:], 1)
    with pytest.raises(ValueError, match='nothing accumulated'):
        finalize_bin_weights(['mu_r'], np.zeros((1, 4), dtype=int), 0)
