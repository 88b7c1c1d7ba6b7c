"""GPU tests of the ensemble modes (ps_modes_*, predictive.EnsembleModes / ModesPosterior) against the numpy
restatement modes_ref: the table of seeded integer fields against the int64 matrix product, exactly, at member counts
around the edges of the matrix-unit tile (16) and of the workgroup tile (64), built by merging -- this settles the
lane map of the f64 matrix instruction; the stored fields, the mean and the combinations bit for bit; the centred
table of model fields within 2 P 2^-53 sqrt(G_ii G_jj) of the exact product, with the live window on and off;
posterior_predictive with modes= and a release plan; and the refusals.  Kalbar wind, the members, weights and helpers
of test_arrival_gpu.py and the four further members of test_representative_gpu.py.  N = 129 has 16 641 = 4 * 4 160 + 1
cells: the last chunk of the cell axis is mostly pad, and the last real cell sits alone in the last word of 64."""
import ctypes as C
import json
import warnings

import numpy as np
import pytest

import modes_ref as R
import test_arrival_gpu as TA
from test_representative_gpu import MORE

pytestmark = pytest.mark.gpu

MEMBERS, WEIGHTS = TA.MEMBERS, TA.WEIGHTS
_pop_model, _evaluate, _fields = TA._pop_model, TA._evaluate, TA._fields
NINE = MEMBERS + MORE
W9 = [1, 3, 1, 2, 1, 2, 1, 1, 4]
EPS = 2.0 ** -53


def _int_fields(seed, n, nslot, N, band=None):
    """n members of [nslot, N, N] whole numbers in 0..7, the last cell non-zero; band: zero outside these rows"""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 8, (n, nslot, N, N)).astype(np.float64)
    if band is not None:
        f[:, :, :band[0]] = 0.0
        f[:, :, band[1]:] = 0.0
    else:
        f[:, :, N - 1, N - 1] = 1.0 + np.arange(n)[:, None] % 7
    return f


def _int_table(f, slot):
    a = f[:, slot].reshape(len(f), -1).astype(np.int64)
    return a @ a.T


def test_the_table_of_integer_fields_is_exact_at_every_tile_edge():
    from parasitoids_amd.predictive import EnsembleModes
    pm = _pop_model(R=64)
    N, days = 129, [1, 4]
    f9 = _int_fields(7, 9, 2, N)
    assert N * N == 4 * 4160 + 1 and (f9[:, :, -1, -1] > 0).all()
    kw = dict(days=days, transform='raw')
    with EnsembleModes(pm, **kw) as E9, EnsembleModes(pm, **kw) as E8, EnsembleModes(pm, **kw) as E5, \
            EnsembleModes(pm, **kw) as E2:
        assert E9.N == N and E9.days == days and E9.transform == 'raw'
        for i in range(9):
            for E, n in ((E9, 9), (E8, 8), (E5, 5), (E2, 2)):
                if i < n:
                    E.add_fields(f9[i], W9[i])
        # 5: inside one matrix tile; 17: one matrix tile + 1; 65: the workgroup tile + 1; 131: two of them + 3
        for M, tail in ((5, E5), (17, E8), (65, E2), (131, E5)):
            reps, rest = divmod(M, 9)
            assert rest == tail.members
            idx = list(range(9)) * reps + list(range(rest))
            with EnsembleModes(pm, **kw) as big:
                for _ in range(reps):
                    big.merge(E9)
                big.merge(tail)
                assert big.members == M and big.weights.tolist() == [W9[i] for i in idx]
                f = f9[idx]
                total = 0
                for s, d in enumerate(days):
                    want = _int_table(f, s)
                    got = big.table(d, centred=False)
                    assert got.dtype == np.float64 and got.shape == (M, M)
                    assert np.array_equal(got, want.astype(np.float64)), (M, d, np.abs(got - want).max())
                    assert np.array_equal(got, got.T)
                    total = total + want
                    big.window(False)
                    assert np.array_equal(big.table(d, centred=False), got), (M, d)
                    big.window(True)
                assert np.array_equal(big.table('all', centred=False), total.astype(np.float64))
                # dropping the last cell changes the table: it was counted
                a = f[:, 0].reshape(M, -1)[:, :-1].astype(np.int64)
                assert not np.array_equal(a @ a.T, _int_table(f, 0))
    pm.close()


def test_the_live_window_skips_only_zeros():
    from parasitoids_amd.predictive import EnsembleModes, Projection
    pm = _pop_model(R=64)
    N, days = 129, [1, 3]
    f = _int_fields(3, 6, 2, N, band=(40, 71))
    with EnsembleModes(pm, days, 'raw') as E:
        for m in range(6):
            E.add_fields(f[m], 1 + m % 3)
        for s, d in enumerate(days):
            want = _int_table(f, s).astype(np.float64)
            assert np.array_equal(E.table(d, centred=False), want)
            E.window(False)
            assert np.array_equal(E.table(d, centred=False), want)
            E.window(True)
        # nothing anywhere: an empty window
        E.reset()
        E.add_fields(np.zeros((2, N, N)), 2)
        assert E.members == 1 and np.array_equal(E.table(1), np.zeros((1, 1)))
    # model fields: on and off inside the same bound, and a projection's outputs as the source
    fields = []
    Wp = np.array([[1.0, 0.5], [0.0, 2.0]])
    with EnsembleModes(pm, days, 'sqrt') as E, Projection(pm, Wp, days) as P, \
            EnsembleModes.for_projection(P, 'raw') as EP:
        pf = []
        for mem, w in zip(MEMBERS, WEIGHTS):
            _evaluate(pm, mem)
            E.add(w)
            P.apply()
            EP.add(w)
            fields.append(_fields(pm, days))
            pf.append(np.array([P.field(e) for e in range(2)]))
        fields = np.array(fields)
        for s, d in enumerate(days):
            A = R.anomalies(R.transform(fields[:, s], 'sqrt'), WEIGHTS)
            ref = R.table(A)
            bound = R.table_bound(ref, N * N)
            on = E.table(d)
            E.window(False)
            off = E.table(d)
            E.window(True)
            for got in (on, off):
                ratio = float((np.abs(got.astype(np.longdouble) - ref) / bound).max())
                assert ratio <= 1.0, 'largest |G - ref| / bound = %g on day %d' % (ratio, d)
                assert np.array_equal(got, got.T)
        assert EP.days == [0, 1] and EP.members == 5
        for m in range(5):
            for e in range(2):
                assert np.array_equal(EP.member(m, e), pf[m][e]), (m, e)
    pm.close()


def test_members_mean_and_combinations_are_bit_for_bit():
    from parasitoids_amd.predictive import EnsembleModes
    pm = _pop_model()
    days = [0, 2, 5]
    fields = []
    with EnsembleModes(pm, days) as E, EnsembleModes(pm, days) as Ea, EnsembleModes(pm, days) as Eb, \
            EnsembleModes(pm, days, 'raw') as Er:
        assert E.N == 257 and E.transform == 'sqrt' and E.member_nbytes == 3 * E.pitch * 8
        for i, (mem, w) in enumerate(zip(MEMBERS, WEIGHTS)):
            _evaluate(pm, mem)
            E.add(w)
            Er.add(w)
            (Ea if i < 2 else Eb).add(w)
            fields.append(_fields(pm, days))
        fields = np.array(fields)
        assert E.members == 5 and E.total_weight == sum(WEIGHTS) and E.weights.tolist() == WEIGHTS
        assert E.capacity >= 5 and E.nbytes >= 5 * E.member_nbytes
        rng = np.random.default_rng(5)
        coef = rng.standard_normal((8, 5))
        for s, d in enumerate(days):
            X = np.sqrt(fields[:, s])
            for m in range(5):
                assert np.array_equal(E.member(m, d), X[m]), (m, d)
                assert np.array_equal(Er.member(m, d), fields[m, s]), (m, d)
            assert (X > 0).sum() > 1000                               # not vacuous
            mu = R.mean(X, WEIGHTS)
            assert np.array_equal(E.mean(d), mu), d
            assert np.array_equal(Er.mean(d), R.mean(fields[:, s], WEIGHTS)), d
            for centred in (True, False):
                A = R.anomalies(X, WEIGHTS, centred)
                for n in (1, 3, 8):
                    got = E.combine(d, coef[:n], centred)
                    assert got.shape == (n, 257, 257)
                    assert np.array_equal(got, R.combine(A, coef[:n])), (d, centred, n)
            once, twice = E.table(d), E.table(d)
            assert np.array_equal(once, twice) and np.array_equal(once, once.T)
        # fields from the host take the same path as the device's: the same bits
        with EnsembleModes(pm, days) as H:
            for m, w in enumerate(WEIGHTS):
                H.add_fields(fields[m], w)
            assert np.array_equal(H.member(3, 2), E.member(3, 2)) and np.array_equal(H.table(5), E.table(5))
        # merge order permutes the table and nothing else
        with EnsembleModes(pm, days) as AB, EnsembleModes(pm, days) as BA:
            AB.merge(Ea)
            AB.merge(Eb)
            BA.merge(Eb)
            BA.merge(Ea)
            perm = [2, 3, 4, 0, 1]
            assert BA.weights.tolist() == [WEIGHTS[i] for i in perm] and Ea.members == 2 and Eb.members == 3
            for d in days:
                assert np.array_equal(AB.table(d, centred=False), E.table(d, centred=False))
                assert np.array_equal(AB.table(d), E.table(d))
                assert np.array_equal(BA.table(d, centred=False), E.table(d, centred=False)[perm][:, perm])
                assert np.array_equal(BA.member(0, d), E.member(2, d))
    pm.close()


@pytest.mark.parametrize('prob_model', [False, True])
def test_the_centred_table_of_model_fields_is_within_the_summation_bound(prob_model):
    """|G_dev - G_ref| <= 2 P 2^-53 sqrt(G_ii G_jj), P = N^2: gamma_P of any summation order through Cauchy-Schwarz,
    the factor 2 for the reference's own rounding.  The largest observed ratio is in the assertion message (and
    printed): 1.5e-4 over these cases."""
    from parasitoids_amd.predictive import EnsembleModes
    pm = _pop_model(prob_model=prob_model)
    days = [2, 5]
    N = 257
    fields = []
    with EnsembleModes(pm, days, 'sqrt') as Es, EnsembleModes(pm, days, 'raw') as Er:
        for mem, w in zip(NINE, W9):
            _evaluate(pm, mem)
            Es.add(w)
            Er.add(w)
            fields.append(_fields(pm, days))
        fields = np.array(fields)
        worst = 0.0
        for E, name in ((Es, 'sqrt'), (Er, 'raw')):
            for s, d in enumerate(days):
                A = R.anomalies(R.transform(fields[:, s], name), W9)
                ref = R.table(A)
                bound = R.table_bound(ref, N * N)
                got = E.table(d)
                assert np.array_equal(got, got.T) and (np.diagonal(got) > 0).all()
                ratio = float((np.abs(got.astype(np.longdouble) - ref) / bound).max())
                worst = max(worst, ratio)
                print('modes table ratio', prob_model, name, d, ratio)
                assert ratio <= 1.0, 'largest |G - ref| / bound = %g (%s, day %d)' % (ratio, name, d)
            tot = E.table('all')
            assert np.array_equal(tot, E.table(days[0]) + E.table(days[1]))
        assert worst > 0.0
    pm.close()


def test_posterior_predictive_with_modes_and_a_release_plan(tmp_path):
    from parasitoids_amd import mcmc
    from parasitoids_amd import predictive as PR
    from test_peak_gpu import _chain
    Rr, N = 64, 129
    res_m = 10000.0 / Rr
    out = [0, 1, 2, 3, 5]
    trace, names = _chain([2, 1, 3, 1, 2])
    chains = [(trace[:5], names), (trace[5:], names)]
    arg = dict(sites=[(0.0, 0.0, 0.6), (13 * res_m, 6 * res_m, 0.5, 2)], days=out)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        one = _pop_model(R=Rr, mode='exact')
        res = PR.posterior_predictive(one, chains, thresholds=[1, 10], sites=arg, modes=dict(days=[1, 3], count=3))
        plain = PR.posterior_predictive(one, chains, thresholds=[1, 10])
    assert plain.modes is None
    assert res.failed == 0 and len(res.runs) == 6
    mp, sp = res.modes, res.sites.modes
    assert mp.days == [1, 3] and mp.planes == [1, 3] and sp.days == out and sp.planes == [1, 3]
    assert mp.count == sp.count == 3 and mp.transform == 'sqrt' and mp.runs == res.runs
    cols = [names.index(m[0]) for m in mcmc.MODEL_BLOCK]
    fields, plan_f, weights = [], [], []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        with PR.ReleaseSites.with_lagged_models(one, arg['sites'], out) as P:
            for ci, first, weight in res.runs:
                P.evaluate(*mcmc.model_args(chains[ci][0][first, cols]))
                fields.append(_fields(one, [1, 3]))
                plan_f.append(np.array([P.field(e) for e in range(len(out))]))
                weights.append(weight)
    assert weights == [2, 1, 2, 1, 1, 2] and mp.weights.tolist() == weights == sp.weights.tolist()
    fields, plan_f = np.array(fields), np.array(plan_f)
    thetas = np.array([chains[ci][0][first, cols] for ci, first, _w in res.runs])
    npz, js = res.save(str(tmp_path / 'a' / 'pp'))
    plain.save(str(tmp_path / 'p' / 'pp'))
    assert not (tmp_path / 'p' / 'pp_modes.npz').exists()
    meta = json.load(open(js))['predictive']
    M, P = 6, N * N
    for name, post, f, fdays, blk in (('', mp, fields, [1, 3], meta['modes']),
                                       ('sites_', sp, plan_f, out, meta['sites']['modes'])):
        keys = {'weights', 'transform', 'days'}
        with np.load(str(tmp_path / 'a' / ('pp_%smodes.npz' % name))) as fz:
            assert fz['weights'].tolist() == weights and str(fz['transform']) == 'sqrt'
            assert fz['days'].tolist() == fdays
            for d in (1, 3):
                s = fdays.index(d)
                X = np.sqrt(f[:, s])
                for m in range(M):
                    assert np.array_equal(post.modes.member(m, d), X[m]), (name, m, d)
                A = R.anomalies(X, weights)
                ref = R.decomposition(A, weights, 3)
                lam, expl = fz['%d_eigenvalues' % d], fz['%d_explained' % d]
                # |dG_ij| <= 2 P eps sqrt(G_ii G_jj) gives |dB_ij| <= 2 P eps sqrt(B_ii B_jj), so |dB|_2 <= |dB|_F <=
                # 2 P eps trace B; with it the eigen-solver's share, 16 M eps trace B (test_modes_cpu)
                dB = (2 * P + 16 * M) * EPS * ref['total_variance']
                assert lam.shape == (3,) and np.all(np.abs(lam - ref['eigenvalues']) <= dB), (lam, ref['eigenvalues'])
                assert np.all(np.diff(lam) < 0) and np.all(lam > 0)
                assert np.array_equal(expl, post.explained(d)) and 0.0 < expl.sum() <= 1.0
                assert np.all(np.abs(expl - ref['explained']) <= 2 * dB / ref['total_variance'])
                assert fz['%d_separated' % d].dtype == np.bool_ and fz['%d_separated' % d].shape == (3,)
                assert np.array_equal(fz['%d_separated' % d], post.separated(d))
                z = fz['%d_scores' % d]
                assert z.shape == (M, 3) and np.array_equal(z, post.scores(d))
                drv = fz['%d_drivers' % d]
                assert drv.shape == (3, len(cols))
                assert np.abs(drv - R.score_drivers(z, thetas, weights)).max() <= 64 * M * EPS
                assert np.array_equal(fz['%d_mean' % d], R.mean(X, weights))
                for k in range(3):
                    pat = fz['%d_mode%d' % (d, k)]
                    assert np.array_equal(pat, post.pattern(k, d))
                    gap = min(abs(ref['spectrum'][k] - ref['spectrum'][j]) for j in range(M) if j != k)
                    tol = (np.sqrt(ref['spectrum'][0] / lam[k]) * 2 * dB / gap + dB / lam[k]
                           + M * EPS * np.sqrt(sum(weights) * ref['total_variance'] / lam[k]))
                    want = np.sqrt(ref['eigenvalues'][k]) * ref['patterns'][k].reshape(N, N)
                    assert np.linalg.norm(pat - want) <= tol * np.sqrt(lam[k]) * 2, (name, d, k)
                    assert abs(np.linalg.norm(post.unit_pattern(k, d)) - 1.0) <= 2 * tol
                    keys.add('%d_mode%d' % (d, k))
                keys |= {'%d_%s' % (d, t) for t in ('eigenvalues', 'explained', 'separated', 'scores', 'drivers',
                                                      'mean')}
                # every mode there is: the member comes back.  Members 2 and 3 are one run cut by the chain boundary, so
                # four directions carry variance; a fifth is kept or not as its eigenvalue, rounding error, falls.  With
                # U the K kept eigenvectors of the computed B' the residual of Y = D^1/2 A / sqrt(W) is its projection on
                # the other M - K, each of squared norm v^T B v = lambda' - v^T dB v <= 2 |dB| (Weyl: |lambda'| <= |dB|
                # where lambda = 0): a member's residual is at most sqrt(W / w_m 2 (M - K) dB), and the sums that form
                # it round at (M + K) eps of the member
                with_all = PR.ModesPosterior(post.modes, count=8, days=[d])
                K = with_all.decomposition(d)['count']
                assert M - 2 <= K <= M - 1
                for m in range(M):
                    back = with_all.reconstruct(m, d)
                    resid = np.linalg.norm(back - X[m])
                    limit = (np.sqrt(sum(weights) / weights[m] * 2 * (M - K) * dB)
                             + 64 * M * EPS * np.linalg.norm(X[m]))
                    print('modes reconstruction', name, d, m, resid, limit)
                    assert resid <= limit, (name, d, m, resid, limit)
                few = post.reconstruct(0, d, modes=1)
                assert np.linalg.norm(few - X[0]) > np.linalg.norm(post.reconstruct(0, d) - X[0]) > 0
            assert set(fz.files) == keys
        assert blk['count'] == 3 and blk['transform'] == 'sqrt' and blk['days'] == fdays and blk['members'] == 6
        assert blk['total_weight'] == 9 and blk['planes_given'] == [1, 3] and blk['given'] == dict(days=[1, 3], count=3)
        assert abs(blk['n_eff'] - 81.0 / 15.0) < 1e-12
        assert [p['plane'] for p in blk['planes']] == [1, 3]
        for p in blk['planes']:
            d = p['plane']
            assert p['count'] == 3 and p['explained'] == post.explained(d).tolist() and sum(p['explained']) <= 1.0
            assert p['separated'] == post.separated(d).tolist()
            assert p['planes_not_patterns'] == [k for k in range(3) if not p['separated'][k]]
            assert p['strongest_driver'] == post.drivers(d)['strongest'] and p['strongest_driver'][0] in names
            for k, ex in enumerate(p['extremes']):
                z = post.scores(d)[:, k]
                assert ex['low']['member'] == int(np.argmin(z)) and ex['high']['member'] == int(np.argmax(z))
                for who in (ex['low'], ex['high']):
                    ci, first, length = res.runs[who['member']]
                    run = who['run']
                    assert (run['chain'], run['first_row'], run['length']) == (ci, first, length)
                    assert list(run['params'].values()) == chains[ci][0][first, cols].tolist()
    # the space-time plane: one decomposition over both days, patterns per day, of unit norm together
    with PR.ModesPosterior(mp.modes, count=2, days='all') as st:
        assert st.planes == ['all']
        e = np.array([st.unit_pattern(0, d, 'all') for d in (1, 3)])
        assert abs(np.sqrt((e * e).sum()) - 1.0) < 1e-8      # the per-day bound above is of the order of 1e-10
        assert np.array_equal(mp.modes.table('all'), mp.modes.table(1) + mp.modes.table(3))
    mp.close()
    for r in (res, plain):
        r.summary.close()
        if r.sites is not None:
            r.sites.close()
    one.close()


def test_refusals():
    from parasitoids_amd import _lib as L
    from parasitoids_amd.predictive import EnsembleModes
    pm = _pop_model(R=64)
    N = 129
    lib = L.load()
    with EnsembleModes(pm, [1, 2], 'raw') as E, EnsembleModes(pm, [1, 2], 'sqrt') as Es, \
            EnsembleModes(pm, [1, 3], 'raw') as Ed:
        f = _int_fields(1, 2, 2, N)
        with pytest.raises(L.HipError, match='nothing accumulated'):
            E.table(1)
        E.add_fields(f[0], 2)
        E.add_fields(f[1])
        out = np.empty((2, 2), dtype=np.float64)
        rc = lib.ps_modes_table(E._h, 0, 1, 1, out.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == L.PS_ERR_BAD_ARG and b'expected' in lib.ps_last_error()          # a stale member count
        for bad in (-1.0, float('nan'), float('inf')):
            g = f[0].copy()
            g[1, 5, 7] = bad
            with pytest.raises(L.HipError) as err:
                E.add_fields(g)
            assert err.value.code == L.PS_ERR_BAD_ARG
        assert E.members == 2 and E.total_weight == 3                                  # nothing stored
        with pytest.raises(ValueError, match='shape'):
            E.add_fields(f[0][:1])
        with pytest.raises(ValueError):
            E.add_fields(f[0], 0)
        with pytest.raises(L.HipError) as err:
            E.merge(Es)                                                                # another transform
        assert err.value.code == L.PS_ERR_BAD_ARG
        with pytest.raises(ValueError, match='different days'):
            E.merge(Ed)
        with pytest.raises(L.HipError):
            E.merge(E)
        cap, held = E.capacity, E.nbytes
        with pytest.raises(L.HipError) as err:
            E.reserve(10 ** 9)                                                         # 2.1e14 B
        assert err.value.code == L.PS_ERR_OOM and 'GB free' in str(err.value)
        assert E.capacity == cap and E.nbytes == held                                  # nothing allocated
        assert np.array_equal(E.table(1, centred=False), _int_table(f, 0).astype(np.float64))
        with pytest.raises(ValueError):
            E.table(3)
        with pytest.raises(ValueError):
            E.combine(1, np.zeros((9, 2)))
        with pytest.raises(ValueError):
            E.combine(1, np.zeros((1, 3)))
        with pytest.raises(L.HipError):
            E.member(2, 1)
    with pytest.raises(ValueError, match='transform'):
        EnsembleModes(pm, [1], 'log')
    with pytest.raises(ValueError, match='at most 8'):
        EnsembleModes(pm, list(range(9)))
    h = C.c_void_p()
    assert lib.ps_modes_create(0, N, 1, 2, C.byref(h)) == L.PS_ERR_BAD_ARG and not h
    assert lib.ps_modes_create(0, N, 9, 1, C.byref(h)) == L.PS_ERR_BAD_ARG and not h
    pm.close()
